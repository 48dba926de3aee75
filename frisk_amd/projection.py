"""Symmetric k-mer proportions of anomalous windows, and their projection and clustering:
PCA, DBSCAN and k-means as the reference runs them through sklearn (L1597-1665), on the GPU (frisk_proj_* / frisk_dbscan /
frisk_kmeans, csrc/proj_kernels.h), and the reference's own exact t-SNE, PY-TSNE (frisk/tsne.py, L1622-1623), on the GPU
(frisk_tsne_*, csrc/tsne_kernels.h), sklearn's metric MDS (L1624-1627) on the GPU (frisk_mds_*, csrc/mds_kernels.h) and sklearn's
IncrementalPCA (L1629-1631) on the GPU, batch by batch with the fit resident on the device (frisk_ipca_*, csrc/ipca_kernels.h),
and sklearn's NMF (L1632-1636: the coordinate-descent solver from the nndsvda start) with X, W and H resident on the device
(frisk_nmf_*, csrc/nmf_kernels.h), and sklearn's SpectralClustering (L1659-1662: rbf affinities, scipy's normalised Laplacian, the
top eigenvectors, k-means) with the n x n matrix resident on the device (frisk_spectral_*, csrc/spectral_kernels.h): affinities,
normalisation and every product of the eigen-iteration are kernels, the iteration's QR and Rayleigh-Ritz on matrices at most 26
columns wide are the host's.  sklearn's TSNE, SKL-TSNE (L1606-1621), runs on the GPU too (frisk_skltsne_*, csrc/skltsne_kernels.h):
both of its methods, the float32 state resident on the device, the stop rule on the host; its barnes_hut method sums the repulsive
term over all pairs (sklearn's angle -> 0 limit) instead of walking a tree at angle = 0.5.

Reference (frisk/__init__.py): computeKmers(sym=True, pcaMode=True) L280-367 counts every valid word AND its
reverse complement for orders pcaMin..pcaMax; scrubMirrors L797-811 keeps one key of each reverse-complement pair
(the first in canonical key order, i.e. codes with c <= revcomp(c)); flattenKmerMap(prop=True) L813-831 turns each
order's kept counts into proportions of their sum and concatenates the orders (loop L1573-1591).
The counting runs on the GPU (per-window forward counts from frisk_scan's count dump); folding and proportions are
host numpy.
"""
import ctypes as C
import logging
import time

import numpy as np

from . import _ffi
from .engine import Engine, table_offset
from .hotpath import kmerString


def revcomp_index(x):
    c = np.arange(4 ** x, dtype=np.int64)
    r = np.zeros_like(c)
    t = c.copy()
    for _ in range(x):
        r = (r << 2) | ((t & 3) ^ 1)        # A<->T, G<->C is XOR 1 on the digit (A,T,G,C = 0,1,2,3)
        t >>= 2
    return r


def mirror_keep(x):
    """codes kept by scrubMirrors at order x, in canonical order."""
    c = np.arange(4 ** x, dtype=np.int64)
    return c[c <= revcomp_index(x)]


def feature_keys(kmin, kmax):
    return [kmerString(int(c), x) for x in range(kmin, kmax + 1) for c in mirror_keep(x)]


def proportions_from_forward(fwd, kmin, kmax):
    """fwd: forward counts in profile layout (orders kmin..kmax) -> the flattenKmerMap(prop=True) vector."""
    out = []
    for x in range(kmin, kmax + 1):
        o = table_offset(kmin, x)
        f = np.asarray(fwd[o:o + 4 ** x], dtype=np.int64)
        sym = f + f[revcomp_index(x)]                      # sym=True: word and reverse complement (L350-351)
        kept = sym[mirror_keep(x)]
        out.append(kept.astype(np.float64) / float(int(kept.sum())))      # float(v) / sum(d.values()) (L822)
    return np.concatenate(out)


def symmetricCounts(labelled_seqs, pcaMin, pcaMax, device=0):
    """(anomLabels, anomCounts) as the reference builds them at L1573-1591: one row of proportions per sequence.
    labelled_seqs: list of (label, sequence)."""
    seqs = [s for _, s in labelled_seqs]
    if not seqs:
        return np.zeros((0, 1), dtype=object), np.zeros((0, len(feature_keys(pcaMin, pcaMax))))
    longest = max(len(s) for s in seqs)
    with Engine(pcaMin, pcaMax, device) as e:
        e.load(seqs)
        e.profile_reset(); e.profile_add(); e.profile_finalize()
        # every sequence as ONE window: with inc = 1 the small-scaffold limit is 1.75 w - 1 >= every length
        res = e.scan(max(longest, 2), 1, scaffolds_all=True, debug=True)
    rows = []
    for i in range(len(seqs)):
        hit = np.nonzero(res.seq_index == i)[0]
        if len(hit) != 1 or not res.kept[hit[0]]:
            raise ValueError("sequence %r has >= 30 %% unresolved bases: no k-mer vector" % (labelled_seqs[i][0],))
        rows.append(proportions_from_forward(res.counts[hit[0]], pcaMin, pcaMax))
    labels = np.array([[lab] for lab, _ in labelled_seqs])
    return labels, np.vstack(rows)


_fallback_logged = False


def windowVectors(engine, seq_index, start, stop, pcaMin, pcaMax, labels=None):
    """symmetricCounts' rows for ranges of the engine's resident batch: row r = the proportions vector of bases
    [start[r], stop[r]) - 0-based, half-open - of resident scaffold seq_index[r], counted, folded and divided on the device
    (Engine.window_vectors, csrc/kvec_kernels.h) with the reference's rules applied as symmetricCounts applies them: a range with
    >= 30 % unresolved bases (L213 / L238) raises the same ValueError, and so does a range without a valid word of some order
    (the reference would divide by zero at L822).  labels: what the errors call the rows (default seq_index:start+1:stop).
    pcaMax above the device kernel's orders: the slices are read back and go through symmetricCounts."""
    global _fallback_logged
    seq_index = np.asarray(seq_index, dtype=np.int64).ravel()
    start = np.asarray(start, dtype=np.int64).ravel()
    stop = np.asarray(stop, dtype=np.int64).ravel()
    n = int(seq_index.size)

    def name(r):
        return labels[r] if labels is not None else "%d:%d:%d" % (seq_index[r], start[r] + 1, stop[r])
    if n == 0:
        return np.zeros((0, len(feature_keys(pcaMin, pcaMax))))
    if pcaMax > _ffi.KVEC_MAX_K:
        if not _fallback_logged:
            logging.getLogger("frisk_amd").info("k-mer vectors of orders %s..%s: above the device kernel's %s, the slices go through "
                                                "the scan's count dump instead", pcaMin, pcaMax, _ffi.KVEC_MAX_K)
            _fallback_logged = True
        seqs = [(name(r), engine.read_seq(int(seq_index[r]), int(start[r]), int(stop[r] - start[r])).decode("ascii")) for r in range(n)]
        return symmetricCounts(seqs, pcaMin, pcaMax, device=getattr(engine, "device", 0))[1]
    X, nn, status = engine.window_vectors(seq_index, start, stop, pcaMin, pcaMax)
    for r in np.nonzero(np.asarray(nn) >= 0.3 * (stop - start))[0].tolist():
        raise ValueError("sequence %r has >= 30 %% unresolved bases: no k-mer vector" % (name(r),))
    for r in np.nonzero(np.asarray(status) & _ffi.KVEC_EMPTY_ORDER)[0].tolist():
        empty = [x for x in range(pcaMin, pcaMax + 1) if int(status[r]) >> (_ffi.KVEC_ORDER_SHIFT + x) & 1]
        raise ValueError("row %d (%r) has no valid word of order %s: no k-mer vector" % (r, name(r), empty[0] if empty else "?"))
    return X


# ------------------------------------------------------------------------------------------------ projection / clustering
DBSCAN_MIN_SAMPLES = 50         # DBSCAN(eps=args.epsDBSCAN, min_samples=50) (L1639)
KMEANS_N_INIT, KMEANS_MAX_ITER, KMEANS_TOL = 20, 500, 1e-4      # KMeans(n_init=20, max_iter=500, tol=0.0001) (L1647-1649)
MDS_N_INIT, MDS_MAX_ITER, MDS_EPS = 5, 500, 1e-3        # MDS(metric=True, n_init=5, max_iter=500, eps=0.001, n_jobs=1) (L1624-1627)
MDS_MAX_N = 50000                   # the dense n x n dissimilarities: 20 GB at the cap


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(name, *args):
    rc = getattr(_ffi.lib(), name)(*args)
    if rc != _ffi.OK:
        raise _ffi.FriskHipError(rc, "%s rejected its input" % name if rc == _ffi.E_ARG else "%s failed" % name)


def _f64(a, ndim):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != ndim:
        raise ValueError("expected a %d-d array, got shape %s" % (ndim, a.shape))
    return a


def cov(X, device=0):
    """(column means, covariance / (n - 1)) of X on the GPU (two-pass centring, FP64)."""
    X = _f64(X, 2)
    n, f = X.shape
    mean, c = np.empty(f), np.empty((f, f))
    _call("frisk_proj_cov", device, _ptr(X), n, f, _ptr(mean), _ptr(c))
    return mean, c


def transform(X, mean, V, device=0):
    """(X - mean) V on the GPU; V: f x d, one component per column."""
    X, mean, V = _f64(X, 2), _f64(mean, 1), _f64(V, 2)
    n, f = X.shape
    Y = np.empty((n, V.shape[1]))
    _call("frisk_proj_transform", device, _ptr(X), _ptr(mean), _ptr(V), n, f, V.shape[1], _ptr(Y))
    return Y


class PCAResult:
    """Y (n x dims), components (dims x f, rows), explained_variance (dims), mean (f); timings in ms (cov / eigh / transform)."""

    def __init__(self, Y, components, explained_variance, mean, timings):
        self.Y, self.components, self.explained_variance, self.mean, self.timings = Y, components, explained_variance, mean, timings


def pca(X, dims, device=0):
    """sklearn's PCA(n_components=dims).fit(X).transform(X) (L1612-1613): covariance on the GPU, its eigendecomposition (one f x f
    torch.linalg.eigh on the same device: on the host, numpy.linalg.eigh took ~2 s at f = 2 772, ten times the covariance - see
    DESIGN.md), the top `dims` components in descending eigenvalue order with sklearn's sign rule (svd_flip(u_based_decision=False):
    the entry of largest absolute value of each component is positive), transform on the GPU."""
    import torch
    X = _f64(X, 2)
    n, f = X.shape
    if not 1 <= dims <= min(n, f):
        raise ValueError("n_components=%d must be between 1 and min(n_samples, n_features)=%d" % (dims, min(n, f)))
    if n < 2:
        raise ValueError("PCA needs at least 2 samples")
    t0 = time.perf_counter()
    mean, c = cov(X, device)
    t1 = time.perf_counter()
    tw, tv = torch.linalg.eigh(torch.from_numpy(c).to(torch.device("cuda", device)))
    w, v = tw.cpu().numpy(), tv.cpu().numpy()
    t2 = time.perf_counter()
    order = np.argsort(w, kind="stable")[::-1][:dims]
    comps = v[:, order].T.copy()
    big = np.argmax(np.abs(comps), axis=1)
    comps *= np.sign(comps[np.arange(dims), big])[:, None]
    Y = transform(X, mean, comps.T, device)
    t3 = time.perf_counter()
    return PCAResult(Y, comps, w[order].copy(), mean, {"cov_ms": 1e3 * (t1 - t0), "eigh_ms": 1e3 * (t2 - t1),
                                                       "transform_ms": 1e3 * (t3 - t2)})


def dbscan(Y, eps, min_samples=DBSCAN_MIN_SAMPLES, device=0):
    """sklearn's DBSCAN(eps, min_samples).fit(Y).labels_ (Euclidean): int32 labels, -1 = noise."""
    Y = _f64(Y, 2)
    labels = np.empty(Y.shape[0], dtype=np.int32)
    _call("frisk_dbscan", device, _ptr(Y), Y.shape[0], Y.shape[1], float(eps), int(min_samples), _ptr(labels))
    return labels


def kmeans_plusplus(Y, k, rs):
    """Greedy k-means++ seeding as sklearn's _kmeans_plusplus (2 + floor(ln k) local trials), drawing from the RandomState rs."""
    n = Y.shape[0]
    trials = 2 + int(np.log(k))
    sq = np.einsum("ij,ij->i", Y, Y)

    def dist2(P):
        d = sq[None, :] - 2.0 * (P @ Y.T) + np.einsum("ij,ij->i", P, P)[:, None]
        return np.maximum(d, 0.0)
    first = rs.choice(n, p=np.full(n, 1.0 / n))
    idx = [int(first)]
    closest = dist2(Y[[first]])[0]
    pot = closest.sum()
    for _ in range(1, k):
        r = rs.uniform(size=trials) * pot
        cand = np.minimum(np.searchsorted(np.cumsum(closest), r), n - 1)
        dc = np.minimum(closest, dist2(Y[cand]))
        pots = dc.sum(axis=1)
        b = int(np.argmin(pots))
        pot, closest = pots[b], dc[b]
        idx.append(int(cand[b]))
    return Y[idx].copy(), np.array(idx)


class KMeansResult:
    def __init__(self, labels, centers, inertia, n_iter):
        self.labels, self.centers, self.inertia, self.n_iter = labels, centers, inertia, n_iter


def kmeans(Y, k, seed=0, n_init=KMEANS_N_INIT, max_iter=KMEANS_MAX_ITER, tol=KMEANS_TOL, device=0, rs=None):
    """sklearn's KMeans(n_clusters=k, init='k-means++', n_init, max_iter, tol).fit(Y) with random_state=seed: n_init Lloyd runs
    on the GPU from k-means++ seeds drawn in turn from one RandomState(seed); the run of lowest inertia is kept (the earliest on
    a tie).  Cluster ids are renumbered by first occurrence in row order.  rs, if given, is the RandomState to draw from instead
    of RandomState(seed) (sklearn's random_state=<instance>: spectral() hands over the one it has already drawn from)."""
    Y = _f64(Y, 2)
    n, d = Y.shape
    if not 1 <= k <= n:
        raise ValueError("n_clusters=%d must be between 1 and n_samples=%d" % (k, n))
    if rs is None:
        rs = np.random.RandomState(seed)
    tol_abs = float(np.mean(np.var(Y, axis=0))) * tol          # sklearn's _tolerance
    best = None
    for _ in range(n_init):
        init, _idx = kmeans_plusplus(Y, k, rs)
        labels, centers = np.empty(n, dtype=np.int32), np.empty((k, d))
        inertia, iters = C.c_double(), C.c_int32()
        _call("frisk_kmeans", device, _ptr(Y), n, d, k, _ptr(np.ascontiguousarray(init)), max_iter, tol_abs, _ptr(labels),
              _ptr(centers), C.byref(inertia), C.byref(iters))
        if best is None or inertia.value < best.inertia:
            best = KMeansResult(labels, centers, inertia.value, iters.value)
    _, first = np.unique(best.labels, return_index=True)
    order = np.unique(best.labels)[np.argsort(first, kind="stable")]
    remap = np.empty(k, dtype=np.int32)
    remap[:] = -1
    remap[order] = np.arange(order.size, dtype=np.int32)
    best.labels = remap[best.labels]
    best.centers = best.centers[order]
    return best


# ------------------------------------------------------------------------------------------------ PY-TSNE
TSNE_ITERATIONS = 1000              # tsne.py max_iter
TSNE_MAX_N = 50000                  # the dense n x n affinities: 20 GB at the cap


class _Handle:
    """A device-side handle of the library (self._h, made by the subclass's frisk_*_create): a context manager that destroys it once."""
    _destroy = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            getattr(_ffi.lib(), self._destroy)(self._h)
            self._h = C.c_void_p()


class TSNE(_Handle):
    """A t-SNE run on the GPU (frisk_tsne_*): X (n x f, f <= 64) already reduced, Y0 (n x dims) the start.  The state stays on
    the device between calls; use as a context manager (or call close())."""

    _destroy = "frisk_tsne_destroy"

    def __init__(self, X, Y0, perplexity=20.0, device=0):
        X, Y0 = _f64(X, 2), _f64(Y0, 2)
        if X.shape[0] != Y0.shape[0]:
            raise ValueError("X has %d rows, Y0 %d" % (X.shape[0], Y0.shape[0]))
        self.n, self.f = X.shape
        self.dims = Y0.shape[1]
        self._h = C.c_void_p()
        _call("frisk_tsne_create", device, _ptr(X), self.n, self.f, float(perplexity), self.dims, _ptr(Y0), C.byref(self._h))

    def affinities(self, q=False):
        """(beta, tries) of every row, plus the n x n q = max(normalised symmetric P, 1e-12 / 4) when q is True."""
        beta, tries = np.empty(self.n), np.empty(self.n, dtype=np.int32)
        qm = np.empty((self.n, self.n)) if q else None
        _call("frisk_tsne_affinities", self._h, _ptr(beta), _ptr(tries), _ptr(qm) if q else None)
        return (beta, tries, qm) if q else (beta, tries)

    def run(self, begin, end):
        """Iterations begin .. end - 1; returns the costs of the t with (t + 1) % 10 == 0 among them."""
        cost = np.empty(max(0, end // 10 - begin // 10))
        _call("frisk_tsne_run", self._h, int(begin), int(end), _ptr(cost))
        return cost

    def get(self):
        """(Y, iY, gains), each n x dims."""
        out = [np.empty((self.n, self.dims)) for _ in range(3)]
        _call("frisk_tsne_get", self._h, *[_ptr(a) for a in out])
        return tuple(out)

    def set(self, Y=None, iY=None, gains=None):
        arrs = [None if a is None else _f64(a, 2) for a in (Y, iY, gains)]
        for a in arrs:
            if a is not None and a.shape != (self.n, self.dims):
                raise ValueError("expected shape %s, got %s" % ((self.n, self.dims), a.shape))
        _call("frisk_tsne_set", self._h, *[None if a is None else _ptr(a) for a in arrs])


class TSNEResult:
    """Y (n x dims), cost (the 100 logged costs, iterations 10, 20, ..., 1000), beta (n), tries (n); timings in ms."""

    def __init__(self, Y, cost, beta, tries, timings):
        self.Y, self.cost, self.beta, self.tries, self.timings = Y, cost, beta, tries, timings


def tsne_input(X, initial_dims=50, device=0):
    """Step 1 of tsne.tsne (its pca(), L83-91): X centred and projected on the top min(initial_dims, f) eigenvectors of its
    covariance (covariance and transform on the GPU, eigh on the same device).  The reference keeps numpy's eig columns, whose
    signs and order differ, but only the pairwise distances of the result are used.  Unlike pca(), any n >= 1 is allowed."""
    import torch
    X = _f64(X, 2)
    f = X.shape[1]
    keep = min(initial_dims, f)
    mean, c = cov(X, device)
    w, v = torch.linalg.eigh(torch.from_numpy(c).to(torch.device("cuda", device)))
    w, v = w.cpu().numpy(), v.cpu().numpy()
    order = np.argsort(w, kind="stable")[::-1][:keep]
    return transform(X, mean, np.ascontiguousarray(v[:, order]), device)


def tsne(X, dims=2, perplexity=20.0, seed=0, initial_dims=50, device=0, log=None):
    """The reference's tsne.tsne(X, dims, initial_dims, perplexity) (L1622-1623) from Y0 = RandomState(seed).randn(n, dims)
    (the reference's draw after np.random.seed(seed)): exact t-SNE, 1000 iterations on the GPU.  log, if given, is called with
    (iteration, cost) every 10 iterations, as the reference logs them.  The trajectory is chaotic: the result matches the
    reference's step by step and in structure, not in its final coordinates."""
    X = _f64(X, 2)
    n = X.shape[0]
    if not 2 <= n <= TSNE_MAX_N:
        raise ValueError("PY-TSNE needs between 2 and %d samples, got %d" % (TSNE_MAX_N, n))
    t0 = time.perf_counter()
    Xp = tsne_input(X, initial_dims, device)
    t1 = time.perf_counter()
    Y0 = np.random.RandomState(seed).randn(n, dims)
    with TSNE(Xp, Y0, perplexity, device) as h:
        beta, tries = h.affinities()
        t2 = time.perf_counter()
        cost = h.run(0, TSNE_ITERATIONS)
        t3 = time.perf_counter()
        Y = h.get()[0]
    if log is not None:
        for k, c in enumerate(cost):
            log(10 * (k + 1), c)
    return TSNEResult(Y, cost, beta, tries, {"pca_ms": 1e3 * (t1 - t0), "affinities_ms": 1e3 * (t2 - t1),
                                             "iterations_ms": 1e3 * (t3 - t2)})


# ------------------------------------------------------------------------------------------------ MDS
class MDS(_Handle):
    """Metric MDS on the GPU (frisk_mds_*): the dissimilarities of X (n x f, any f >= 1) stay on the device, and each run() is one
    SMACOF start against them.  Use as a context manager (or call close())."""

    _destroy = "frisk_mds_destroy"

    def __init__(self, X, dims=2, device=0):
        X = _f64(X, 2)
        self.n, self.f = X.shape
        self.dims = int(dims)
        self._h = C.c_void_p()
        _call("frisk_mds_create", device, _ptr(X), self.n, self.f, self.dims, C.byref(self._h))

    def dissimilarities(self):
        """The n x n D (direct-difference Euclidean distances of the rows of X)."""
        D = np.empty((self.n, self.n))
        _call("frisk_mds_dissimilarities", self._h, _ptr(D))
        return D

    def run(self, Y0, max_iter=MDS_MAX_ITER, eps=MDS_EPS):
        """sklearn's _smacof_single(D, metric=True, init=Y0, max_iter, eps): (Y, raw stress, iterations, stress after each
        iteration)."""
        Y0 = _f64(Y0, 2)
        if Y0.shape != (self.n, self.dims):
            raise ValueError("expected a start of shape %s, got %s" % ((self.n, self.dims), Y0.shape))
        Y, trace = np.empty_like(Y0), np.empty(max(1, int(max_iter)))
        stress, iters = C.c_double(), C.c_int32()
        _call("frisk_mds_run", self._h, _ptr(Y0), int(max_iter), float(eps), _ptr(Y), C.byref(stress), C.byref(iters),
              _ptr(trace))
        return Y, stress.value, iters.value, trace[:iters.value].copy()


class MDSResult:
    """Y (n x dims) of the best start, its raw stress and iterations, best_start (0-based), the stresses and n_iters of every
    start; timings in ms (dissimilarities / smacof)."""

    def __init__(self, Y, stress, n_iter, best_start, stresses, n_iters, timings):
        self.Y, self.stress, self.n_iter, self.best_start = Y, stress, n_iter, best_start
        self.stresses, self.n_iters, self.timings = stresses, n_iters, timings


def mds(X, dims=2, seed=0, n_init=MDS_N_INIT, max_iter=MDS_MAX_ITER, eps=MDS_EPS, device=0):
    """sklearn's MDS(n_components=dims, metric=True, n_init, max_iter, eps, n_jobs=1, dissimilarity='euclidean',
    random_state=seed).fit_transform(X) (L1624-1627): D on the GPU from direct differences, then n_init SMACOF runs on the GPU
    from starts drawn in turn from one RandomState(seed) (uniform on [0, 1)); the run of lowest raw stress is kept (the earliest
    on a tie)."""
    X = _f64(X, 2)
    n = X.shape[0]
    if not 2 <= n <= MDS_MAX_N:
        raise ValueError("MDS needs between 2 and %d samples, got %d" % (MDS_MAX_N, n))
    rs = np.random.RandomState(seed)
    t0 = time.perf_counter()
    with MDS(X, dims, device) as h:
        t1 = time.perf_counter()
        best, stresses, n_iters = None, [], []
        for k in range(n_init):
            Y, stress, iters, _ = h.run(rs.uniform(size=n * dims).reshape(n, dims), max_iter, eps)
            stresses.append(stress)
            n_iters.append(iters)
            if best is None or stress < best[1]:
                best = (Y, stress, iters, k)
        t2 = time.perf_counter()
    return MDSResult(best[0], best[1], best[2], best[3], stresses, n_iters,
                     {"dissimilarities_ms": 1e3 * (t1 - t0), "smacof_ms": 1e3 * (t2 - t1)})


# ------------------------------------------------------------------------------------------------ IncrementalPCA
def gen_batches(n, batch_size, min_batch_size=0):
    """sklearn.utils.gen_batches as (start, stop) pairs: full batches of batch_size rows; a tail shorter than min_batch_size
    rows is merged into the batch before it."""
    out, start = [], 0
    for _ in range(int(n // batch_size)):
        end = start + batch_size
        if end + min_batch_size > n:
            continue
        out.append((start, end))
        start = end
    if start < n:
        out.append((start, n))
    return out


class IncrementalPCA(_Handle):
    """sklearn's IncrementalPCA(n_components=dims, whiten=False) on the GPU (frisk_ipca_*): the fit (rows seen, mean, variance,
    singular values, components) stays on the device between partial_fit calls, so X is only ever needed one batch at a time.
    Per batch the device computes sklearn's mean / variance update and the Gram matrix G = AT A of sklearn's stacked matrix A;
    the right singular vectors of A are the eigenvectors of G (one f x f torch.linalg.eigh on the same device, as pca()), the
    top `dims` in descending order with sklearn's sign rule.  Because only `dims` components survive each batch, a fit of more
    than one batch is not the PCA of X.  Use as a context manager (or call close())."""

    _destroy = "frisk_ipca_destroy"

    def __init__(self, f, dims, device=0):
        self.f, self.dims, self.device = int(f), int(dims), device
        if not 1 <= self.dims <= self.f:
            raise ValueError("n_components=%r invalid for n_features=%d, need more rows than columns for IncrementalPCA processing"
                             % (dims, f))
        self._h = C.c_void_p()
        _call("frisk_ipca_create", device, self.f, self.dims, C.byref(self._h))
        self.n_samples_seen_ = 0
        self.explained_variance_ = self.explained_variance_ratio_ = self.noise_variance_ = None
        self.timings = {"stats_ms": 0.0, "gram_ms": 0.0, "eigh_ms": 0.0}       # of the last partial_fit

    def state(self):
        """(n_samples_seen_, mean_, var_, singular_values_, components_) of the fit on the device; the arrays are None before
        the first batch."""
        seen = C.c_int64()
        _call("frisk_ipca_get", self._h, C.byref(seen), None, None, None, None)
        if seen.value == 0:
            return 0, None, None, None, None
        mean, var, S, Vt = np.empty(self.f), np.empty(self.f), np.empty(self.dims), np.empty((self.dims, self.f))
        _call("frisk_ipca_get", self._h, None, _ptr(mean), _ptr(var), _ptr(S), _ptr(Vt))
        return seen.value, mean, var, S, Vt

    def set_state(self, n_samples_seen, mean=None, var=None, singular_values=None, components=None):
        """Replace the fit on the device (n_samples_seen = 0: unfitted).  The derived attributes (explained_variance_, ...) are
        those of a batch and are cleared."""
        n = int(n_samples_seen)
        if n < 0:
            raise ValueError("n_samples_seen must be >= 0")
        if n == 0:
            _call("frisk_ipca_set", self._h, 0, None, None, None, None)
        else:
            mean, var, S, Vt = _f64(mean, 1), _f64(var, 1), _f64(singular_values, 1), _f64(components, 2)
            if mean.shape != (self.f,) or var.shape != (self.f,) or S.shape != (self.dims,) or Vt.shape != (self.dims, self.f):
                raise ValueError("state arrays do not have the shapes of f = %d, dims = %d" % (self.f, self.dims))
            _call("frisk_ipca_set", self._h, n, _ptr(mean), _ptr(var), _ptr(S), _ptr(Vt))
        self.n_samples_seen_ = n
        self.explained_variance_ = self.explained_variance_ratio_ = self.noise_variance_ = None

    mean_ = property(lambda self: self.state()[1])
    var_ = property(lambda self: self.state()[2])
    singular_values_ = property(lambda self: self.state()[3])
    components_ = property(lambda self: self.state()[4])

    def partial_fit(self, X):
        import torch
        X = _f64(X, 2)
        b, f = X.shape
        d = self.dims
        if f != self.f:
            raise ValueError("X has %d features, the fit %d" % (f, self.f))
        first = self.n_samples_seen_ == 0
        if first and d > b:
            raise ValueError("n_components=%d must be less or equal to the batch number of samples %d for the first partial_fit "
                             "call." % (d, b))
        if b < 1:
            raise ValueError("an empty batch")
        G = np.empty((f, f))
        _call("frisk_ipca_gram", self._h, _ptr(X), b, _ptr(G))
        t0 = time.perf_counter()
        tw, tv = torch.linalg.eigh(torch.from_numpy(G).to(torch.device("cuda", self.device)))
        w, v = tw.cpu().numpy(), tv.cpu().numpy()
        t1 = time.perf_counter()
        order = np.argsort(w, kind="stable")[::-1][:d]
        comps = v[:, order].T.copy()
        big = np.argmax(np.abs(comps), axis=1)
        comps *= np.sign(comps[np.arange(d), big])[:, None]
        lam = np.maximum(w[order], 0.0)
        S = np.sqrt(lam)
        _call("frisk_ipca_commit", self._h, _ptr(S), _ptr(comps))
        total = self.n_samples_seen_ + b
        var = self.state()[2]
        n_values = min(b if first else d + b + 1, f)            # singular values of A
        trace = float(np.cumsum(np.diagonal(G))[-1])            # sum of all of them squared, in index order
        with np.errstate(divide="ignore", invalid="ignore"):
            self.explained_variance_ = S ** 2 / (total - 1)
            self.explained_variance_ratio_ = S ** 2 / np.sum(var * total)
            if d in (b, f):
                self.noise_variance_ = 0.0
            else:
                self.noise_variance_ = max(trace - float(np.cumsum(lam)[-1]), 0.0) / (total - 1) / (n_values - d)
        self.n_samples_seen_ = total
        ms = _ffi.lib().frisk_ipca_last_ms
        self.timings = {"upload_ms": ms(self._h, 0), "stats_ms": ms(self._h, 1), "gram_ms": ms(self._h, 2),
                        "eigh_ms": 1e3 * (t1 - t0)}
        return self

    def transform(self, X):
        """(X - mean_) components_.T on the GPU, any number of rows."""
        X = _f64(X, 2)
        if X.shape[1] != self.f:
            raise ValueError("X has %d features, the fit %d" % (X.shape[1], self.f))
        Y = np.empty((X.shape[0], self.dims))
        if X.shape[0]:
            _call("frisk_ipca_transform", self._h, _ptr(X), X.shape[0], _ptr(Y))
        return Y


class IncrementalPCAResult:
    """Y (n x dims) and the fit under sklearn's names (components_ dims x f, singular_values_, mean_, var_, n_samples_seen_,
    explained_variance_, explained_variance_ratio_, noise_variance_), batch_sizes, timings in ms (statistics + Gram with the
    batch traffic / eigh / transform; kernels: the device time of statistics + stack and of the Gram kernels alone)."""

    def __init__(self, Y, fit, batch_sizes, timings):
        self.Y, self.batch_sizes, self.timings = Y, batch_sizes, timings
        self.n_samples_seen_, self.mean_, self.var_, self.singular_values_, self.components_ = fit.state()
        self.explained_variance_, self.explained_variance_ratio_ = fit.explained_variance_, fit.explained_variance_ratio_
        self.noise_variance_ = fit.noise_variance_


def incremental_pca(X, dims, batch_size=None, device=0):
    """sklearn's IncrementalPCA(n_components=dims, batch_size=batch_size).fit(X).transform(X) (L1629-1631): batches of
    batch_size rows (None: 5 * n_features), a tail shorter than dims rows merged into the batch before it."""
    X = _f64(X, 2)
    n, f = X.shape
    size = 5 * f if batch_size is None else int(batch_size)
    if size < 1:
        raise ValueError("batch_size must be >= 1")
    if n < 1:
        raise ValueError("IncrementalPCA needs at least 1 sample")
    batches = gen_batches(n, size, dims)
    t = {"stats_gram_ms": 0.0, "eigh_ms": 0.0, "transform_ms": 0.0, "stats_kernels_ms": 0.0, "gram_kernels_ms": 0.0}
    with IncrementalPCA(f, dims, device) as fit:
        for lo, hi in batches:
            t0 = time.perf_counter()
            fit.partial_fit(X[lo:hi])
            t["stats_gram_ms"] += 1e3 * (time.perf_counter() - t0) - fit.timings["eigh_ms"]
            t["eigh_ms"] += fit.timings["eigh_ms"]
            t["stats_kernels_ms"] += fit.timings["stats_ms"]
            t["gram_kernels_ms"] += fit.timings["gram_ms"]
        t0 = time.perf_counter()
        Y = fit.transform(X)
        t["transform_ms"] = 1e3 * (time.perf_counter() - t0)
        return IncrementalPCAResult(Y, fit, [hi - lo for lo, hi in batches], t)


# ------------------------------------------------------------------------------------------------ NMF
NMF_TOL, NMF_MAX_ITER = 1e-4, 200       # NMF(init=None, solver='cd', tol=0.0001, max_iter=200, shuffle=False) (L1633-1635)
NMF_MAX_DIMS, NMF_MAX_P = 16, 26        # components; columns of one product (d plus the range finder's 10 oversamples)
NMF_OVERSAMPLES, NMF_INIT_EPS = 10, 1e-6


class NMF(_Handle):
    """An NMF problem on the GPU (frisk_nmf_*): X (n x f, non-negative) stays on the device with W (n x dims) and H (dims x f).
    The caller drives the iterations: step() is one pass of sklearn's coordinate descent and returns its violation.  Use as a
    context manager (or call close())."""

    _destroy = "frisk_nmf_destroy"

    def __init__(self, X, dims=2, device=0):
        X = _f64(X, 2)
        self.n, self.f = X.shape
        self.dims = int(dims)
        self._h = C.c_void_p()
        _call("frisk_nmf_create", device, _ptr(X), self.n, self.f, self.dims, C.byref(self._h))

    def xq(self, Q):
        """X Q for Q (f x p, p <= 26)."""
        Q = _f64(Q, 2)
        if Q.shape[0] != self.f:
            raise ValueError("expected %d rows, got shape %s" % (self.f, Q.shape))
        Y = np.empty((self.n, Q.shape[1]))
        _call("frisk_nmf_xq", self._h, _ptr(Q), Q.shape[1], _ptr(Y))
        return Y

    def xtq(self, Q):
        """XT Q for Q (n x p, p <= 26)."""
        Q = _f64(Q, 2)
        if Q.shape[0] != self.n:
            raise ValueError("expected %d rows, got shape %s" % (self.n, Q.shape))
        Z = np.empty((self.f, Q.shape[1]))
        _call("frisk_nmf_xtq", self._h, _ptr(Q), Q.shape[1], _ptr(Z))
        return Z

    def set(self, W=None, H=None):
        W, H = (None if W is None else _f64(W, 2)), (None if H is None else _f64(H, 2))
        if W is not None and W.shape != (self.n, self.dims):
            raise ValueError("expected W of shape %s, got %s" % ((self.n, self.dims), W.shape))
        if H is not None and H.shape != (self.dims, self.f):
            raise ValueError("expected H of shape %s, got %s" % ((self.dims, self.f), H.shape))
        _call("frisk_nmf_set", self._h, None if W is None else _ptr(W), None if H is None else _ptr(H))

    def get(self):
        """(W, H): n x dims and dims x f."""
        W, H = np.empty((self.n, self.dims)), np.empty((self.dims, self.f))
        _call("frisk_nmf_get", self._h, _ptr(W), _ptr(H))
        return W, H

    def step(self, update_H=True):
        """One iteration on the state on the device: the W sweep, then the H sweep when update_H.  Returns the violation."""
        v = C.c_double()
        _call("frisk_nmf_step", self._h, None, None, 1 if update_H else 0, C.byref(v))
        return v.value

    def transform_prepare(self):
        """Freeze H HT and X HT of the current H for the steps of a transform."""
        _call("frisk_nmf_transform_prepare", self._h)

    def last_ms(self):
        """Device ms of the last call: (X Q or X HT, XT Q or XT W, the whole last step)."""
        ms = _ffi.lib().frisk_nmf_last_ms
        return ms(self._h, 0), ms(self._h, 1), ms(self._h, 2)

    def iterate(self, update_H, tol=NMF_TOL, max_iter=NMF_MAX_ITER):
        """sklearn's _fit_coordinate_descent loop and stop rule from the state on the device: (iterations, violation ratios)."""
        ratios, init, it = [], None, 0
        for it in range(1, int(max_iter) + 1):
            v = self.step(update_H)
            if it == 1:
                init = v
            if init == 0:
                break
            ratios.append(v / init)
            if v / init <= tol:
                break
        return it, ratios


def nmf_randomized_svd(h, dims, seed=0):
    """sklearn.utils.extmath._randomized_svd(X, dims, random_state=seed) (n_oversamples = 10, n_iter and transpose 'auto', the LU
    power-iteration normaliser, svd_flip) with every product against X on the GPU through the handle h; the LU, QR and the small
    SVD are scipy's on the host, on matrices at most dims + 10 wide.  Returns (U n x dims, S, V dims x f)."""
    from scipy import linalg
    n, f = h.n, h.f
    n_iter = 7 if dims < 0.1 * min(n, f) else 4
    transpose = n < f                                   # M = XT then: the range finder runs on the smaller side
    mul, mul_t = (h.xtq, h.xq) if transpose else (h.xq, h.xtq)         # M Q and MT Q
    Q = np.random.RandomState(seed).normal(size=(n if transpose else f, dims + NMF_OVERSAMPLES))
    for _ in range(n_iter):
        Q, _u = linalg.lu(mul(Q), permute_l=True, check_finite=False)
        Q, _u = linalg.lu(mul_t(Q), permute_l=True, check_finite=False)
    Q, _r = linalg.qr(mul(Q), mode="economic", check_finite=False)
    B = mul_t(Q).T                                      # QT M
    Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    if not transpose:                                   # svd_flip(U, Vt): the largest |entry| of each column of U positive
        signs = np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])
    else:                                               # svd_flip(U, Vt, u_based_decision=False): of each row of Vt
        signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    U, Vt = U * signs[None, :], Vt * signs[:, None]
    if transpose:
        return Vt[:dims].T, s[:dims], U[:, :dims].T
    return U[:, :dims], s[:dims], Vt[:dims]


def nmf_nndsvda(U, S, V, avg):
    """The NNDSVD split of sklearn's _initialize_nmf on the triplets (U, S, V), entries below 1e-6 zeroed, zeros set to avg."""
    def norm(x):
        return np.sqrt(np.dot(x, x))
    W, H = np.zeros_like(U), np.zeros_like(V)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, U.shape[1]):
        x, y = U[:, j], V[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm, x_n_nrm, y_n_nrm = norm(x_p), norm(y_p), norm(x_n), norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        if m_p > m_n:
            u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
        else:
            u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    W[W < NMF_INIT_EPS] = 0
    H[H < NMF_INIT_EPS] = 0
    W[W == 0] = avg
    H[H == 0] = avg
    return W, H


def nmf_init(h, X, dims, seed=0):
    """sklearn's _initialize_nmf(X, dims, init=None, random_state=seed): nndsvda when dims <= min(n, f), else 'random' (H drawn
    first, then W).  Returns (W0, H0)."""
    n, f = X.shape
    if dims <= min(n, f):
        U, S, V = nmf_randomized_svd(h, dims, seed)
        return nmf_nndsvda(U, S, V, X.mean())
    avg = np.sqrt(X.mean() / dims)
    rs = np.random.RandomState(seed)
    H = avg * rs.standard_normal(size=(dims, f))
    W = avg * rs.standard_normal(size=(n, dims))
    return np.abs(W), np.abs(H)


class NMFResult:
    """Y (n x dims, the transform of X), components (dims x f), n_iter and transform_n_iter, violation_ratios (violation /
    violation of the first iteration, per fit iteration), W0 and H0 (the start); timings in ms (init / fit / transform)."""

    def __init__(self, Y, components, n_iter, transform_n_iter, violation_ratios, W0, H0, timings):
        self.Y, self.components, self.n_iter, self.transform_n_iter = Y, components, n_iter, transform_n_iter
        self.violation_ratios, self.W0, self.H0, self.timings = violation_ratios, W0, H0, timings


def nmf(X, dims, seed=0, tol=NMF_TOL, max_iter=NMF_MAX_ITER, device=0):
    """sklearn's NMF(n_components=dims, init=None, solver='cd', tol, max_iter, shuffle=False, random_state=seed).fit(X)
    .transform(X) (L1632-1636).  The start is sklearn's (nmf_init); every iteration of the fit and of the transform (W from zeros,
    H fixed) is one step on the GPU, the stop rule evaluated on the host in double.  Clustering this projection is not offered by
    the CLI yet (cli.PROJECTIONS_UNCLUSTERED).  Components that come out of the fit all zero (an all-zero X) raise the ValueError of
    sklearn's transform."""
    X = _f64(X, 2)
    n, f = X.shape
    dims = int(dims)
    if n < 1 or f < 1:
        raise ValueError("NMF needs at least 1 sample and 1 feature, got shape %s" % (X.shape,))
    if not 1 <= dims <= NMF_MAX_DIMS:
        raise ValueError("n_components=%d must be between 1 and %d" % (dims, NMF_MAX_DIMS))
    if not np.all(np.isfinite(X)) or X.min() < 0:
        raise ValueError("Negative values in data passed to NMF (input X)" if np.all(np.isfinite(X)) else "X is not finite")
    t0 = time.perf_counter()
    with NMF(X, dims, device) as h:
        W0, H0 = nmf_init(h, X, dims, seed)
        t1 = time.perf_counter()
        h.set(W0, H0)
        n_iter, ratios = h.iterate(True, tol, max_iter)
        if n_iter == max_iter and tol > 0:              # sklearn's ConvergenceWarning
            logging.getLogger(__name__).warning("NMF: maximum number of iterations %d reached. Increase it to improve "
                                                "convergence.", max_iter)
        _W, H = h.get()
        if not H.any():                                 # sklearn's transform: _check_init(H, ..., "NMF (input H)")
            raise ValueError("Array passed to NMF (input H) is full of zeros.")
        t2 = time.perf_counter()
        h.set(W=np.zeros((n, dims)))
        h.transform_prepare()
        t_iter, _r = h.iterate(False, tol, max_iter)
        if t_iter == max_iter and tol > 0:
            logging.getLogger(__name__).warning("NMF transform: maximum number of iterations %d reached. Increase it to "
                                                "improve convergence.", max_iter)
        Y = h.get()[0]
        t3 = time.perf_counter()
    return NMFResult(Y, H, n_iter, t_iter, ratios, W0, H0,
                     {"init_ms": 1e3 * (t1 - t0), "fit_ms": 1e3 * (t2 - t1), "transform_ms": 1e3 * (t3 - t2)})


# ------------------------------------------------------------------------------------------------ spectral clustering
SPECTRAL_GAMMA, SPECTRAL_N_INIT = 1.0, 20       # SpectralClustering(gamma=1.0, affinity='rbf', n_init=20) (L1659-1662)
SPECTRAL_KMEANS_MAX_ITER = 300                  # sklearn's k_means default, which spectral_clustering leaves alone
SPECTRAL_MAX_N = 50000                          # the dense n x n matrix: 20 GB at the cap
SPECTRAL_MAX_K, SPECTRAL_MAX_P, SPECTRAL_GUARD = 16, 26, 10     # clusters; columns of one product = k + the guard columns
# The stop rule of spectral_embedding: every one of the first k Ritz pairs (theta, v) of M + I has |(M + I) v - theta v|_2 <= tol.
# With residuals r the computed invariant subspace is within sin(angle) <= r sqrt(k) / gap_k of the true one (Davis-Kahan), so
# at the smallest gap the goldens allow, 0.1, tol = 1e-10 pins it to 4e-9: far below anything k-means can see, and useful as a
# test bound.  The floor is the rounding of one product, about n eps64 |M| |Q| = 1.1e-11 at the cap n = 50 000 (rows of |M| |Q| are
# at most 1): tol sits a factor 9 above it, so the iteration cannot stall short of the rule.
SPECTRAL_TOL = 1e-10
# Subspace iteration on M + I (eigenvalues in [0, 2]) contracts the k-th Ritz vector's error by (1 + lambda_{p+1}) / (1 + lambda_k)
# per step.  Worst case: the guard columns buy nothing (lambda_{p+1} = lambda_{k+1}), the gap is the smallest allowed,
# lambda_k - lambda_{k+1} = 0.1, and lambda_k = 1 (the rate 1 - 0.1 / (1 + lambda_k) is largest there): 1.9 / 2 = 0.95 per step,
# so from an error of order 1 to 1e-10 takes ln(1e10) / -ln(0.95) = 449 steps.  500 leaves a tenth in hand.
SPECTRAL_MAX_ITER = 500


class Spectral(_Handle):
    """The dense part of spectral clustering on the GPU (frisk_spectral_*): from Y (n x d, d <= 64) the rbf affinities, scipy's
    normalisation and M = D^-1/2 A0 D^-1/2, which stays on the device; each mq() is one product against it.  Use as a context
    manager (or call close())."""

    _destroy = "frisk_spectral_destroy"

    def __init__(self, Y, gamma=SPECTRAL_GAMMA, device=0):
        Y = _f64(Y, 2)
        self.n, self.d = Y.shape
        self.gamma = float(gamma)
        self.timings = {"products": 0, "product_ms": 0.0, "product_wall_ms": 0.0, "host_ms": 0.0}   # of the last spectral_embedding
        self._h = C.c_void_p()
        _call("frisk_spectral_create", device, _ptr(Y), self.n, self.d, self.gamma, C.byref(self._h))

    def affinity(self):
        """The n x n A0 = exp(-gamma |y_i - y_j|^2) with a zero diagonal (recomputed; M is restored afterwards)."""
        A = np.empty((self.n, self.n))
        _call("frisk_spectral_affinity", self._h, _ptr(A))
        return A

    def degrees(self):
        """(dd, n_isolated): dd = sqrt(column sums of A0), a zero sum replaced by 1, and the number of such points."""
        dd, iso = np.empty(self.n), C.c_int64()
        _call("frisk_spectral_degrees", self._h, _ptr(dd), C.byref(iso))
        return dd, iso.value

    def matrix(self):
        """The n x n M = (A0 / dd) / dd[:, None], exactly symmetric."""
        M = np.empty((self.n, self.n))
        _call("frisk_spectral_matrix", self._h, _ptr(M))
        return M

    def mq(self, Q):
        """M Q for Q (n x p, p <= 26)."""
        Q = _f64(Q, 2)
        if Q.shape[0] != self.n:
            raise ValueError("expected %d rows, got shape %s" % (self.n, Q.shape))
        Z = np.empty((self.n, Q.shape[1]))
        _call("frisk_spectral_mq", self._h, _ptr(Q), Q.shape[1], _ptr(Z))
        return Z

    def last_ms(self):
        """Device ms: (the last affinity computation, degrees + normalisation, the last product)."""
        ms = _ffi.lib().frisk_spectral_last_ms
        return ms(self._h, 0), ms(self._h, 1), ms(self._h, 2)


def spectral_embedding(h, k, seed=0, tol=SPECTRAL_TOL, max_iter=SPECTRAL_MAX_ITER):
    """sklearn.manifold.spectral_embedding(affinity, n_components=k, norm_laplacian=True, drop_first=False) on the handle h: the k
    eigenpairs of M of largest ALGEBRAIC eigenvalue, by block subspace iteration with Rayleigh-Ritz on M + I.  (M has zero trace
    and eigenvalues down to -1 - two mutually close points far from the rest give +-1 - so unshifted iteration would find the
    largest magnitudes; M + I is positive semi-definite.)  p = min(k + 10, n) columns from Q0 = qr(RandomState(seed).uniform(-1, 1,
    (n, p))).  Each step is one product on the GPU, Z = M Q + Q, and on the host, on matrices p wide: B = QT Z symmetrised, its
    eigenpairs (theta, S) in descending order, V = Q S, R = Z S - V theta; stop when the largest 2-norm of the first k columns of
    R is <= tol, else Q = qr(Z S).  At max_iter a warning is logged and the current Ritz pairs are returned.  Then sklearn's steps:
    each vector divided by dd, its entry of largest absolute value made positive (_deterministic_vector_sign_flip), transposed.
    Returns (E n x k, eigenvalues of M (k, descending), residuals (k), iterations); h.timings has the device time of the products,
    their wall-clock with the transfers, and the host's linear algebra."""
    n = h.n
    k = int(k)
    if not 1 <= k <= min(SPECTRAL_MAX_K, n):
        raise ValueError("n_components=%d must be between 1 and min(%d, n_samples=%d)" % (k, SPECTRAL_MAX_K, n))
    p = min(k + SPECTRAL_GUARD, n)
    t = {"products": 0, "product_ms": 0.0, "product_wall_ms": 0.0, "host_ms": 0.0}
    t0 = time.perf_counter()
    Q = np.linalg.qr(np.random.RandomState(seed).uniform(-1, 1, (n, p)))[0]
    it = 0
    while True:
        it += 1
        t1 = time.perf_counter()
        t["host_ms"] += 1e3 * (t1 - t0)
        Z = h.mq(Q)
        t0 = time.perf_counter()
        t["products"] += 1
        t["product_wall_ms"] += 1e3 * (t0 - t1)
        t["product_ms"] += h.last_ms()[2]
        MQ = Z
        Z = MQ + Q
        B = Q.T @ Z
        theta, S = np.linalg.eigh(0.5 * (B + B.T))
        theta, S = theta[::-1], S[:, ::-1]
        ZS = Z @ S
        V = Q @ S
        res = np.sqrt(np.sum((ZS - V * theta) ** 2, axis=0))[:k]
        if res.max() <= tol:
            break
        if it >= max_iter:
            logging.getLogger(__name__).warning("spectral embedding: residual %.3g above %.3g after %d iterations; the current "
                                                "Ritz vectors are used.", res.max(), tol, it)
            break
        Q = np.linalg.qr(ZS)[0]
    # the eigenvalues of M as Rayleigh quotients of the Ritz vectors against M itself (theta - 1 carries the rounding of the shift)
    lam = np.sum(V[:, :k] * (MQ @ S[:, :k]), axis=0) / np.sum(V[:, :k] * V[:, :k], axis=0)
    dd, _iso = h.degrees()
    E = V[:, :k].T / dd
    big = np.argmax(np.abs(E), axis=1)
    E *= np.sign(E[np.arange(k), big])[:, None]
    t["host_ms"] += 1e3 * (time.perf_counter() - t0)
    h.timings = t
    return np.ascontiguousarray(E.T), lam, res, it


class SpectralResult:
    """labels (n, renumbered by first occurrence), embedding (n x k), eigenvalues of M (k, descending), residuals (k), n_iter,
    n_isolated, timings in ms (affinity and normalise: device; products: device, products_wall with the transfers, host: the
    iteration's linear algebra; embedding and kmeans: wall-clock)."""

    def __init__(self, labels, embedding, eigenvalues, residuals, n_iter, n_isolated, timings):
        self.labels, self.embedding, self.eigenvalues, self.residuals = labels, embedding, eigenvalues, residuals
        self.n_iter, self.n_isolated, self.timings = n_iter, n_isolated, timings


def spectral(Y, k, seed=0, gamma=SPECTRAL_GAMMA, n_init=SPECTRAL_N_INIT, device=0):
    """sklearn's SpectralClustering(n_clusters=k, eigen_solver=None, n_init, gamma, affinity='rbf', eigen_tol=0.0, assign_labels=
    'kmeans', random_state=seed).fit_predict(Y) (L1659-1662): affinities, normalisation and every product of the eigen-iteration
    on the GPU (Spectral, spectral_embedding), then k_means(embedding, k, n_init, max_iter=300) on the GPU.  One rs = RandomState(
    seed) serves as in sklearn: the n draws ARPACK's start vector takes there are discarded, then k-means draws from the same rs.
    The eigenvectors are ARPACK's up to a rotation among (nearly) equal eigenvalues, which k-means cannot see.  A point whose every
    affinity underflows to 0 (n_isolated > 0) certainly disconnects the graph and logs sklearn's warning; connectivity proper
    (sklearn's _graph_is_connected) is not tested, so a graph disconnected by exact zeros between groups of points goes unwarned."""
    Y = _f64(Y, 2)
    n = Y.shape[0]
    k = int(k)
    if not 2 <= n <= SPECTRAL_MAX_N:
        raise ValueError("SPECTRAL needs between 2 and %d samples, got %d" % (SPECTRAL_MAX_N, n))
    if not (1 <= k <= SPECTRAL_MAX_K and k < n):
        raise ValueError("n_clusters=%d must be between 1 and %d and below n_samples=%d" % (k, SPECTRAL_MAX_K, n))
    rs = np.random.RandomState(seed)
    rs.uniform(-1, 1, n)                                # sklearn's _init_arpack_v0
    t0 = time.perf_counter()
    with Spectral(Y, gamma, device) as h:
        _dd, n_isolated = h.degrees()
        aff_ms, norm_ms, _ = h.last_ms()
        if n_isolated:
            logging.getLogger(__name__).warning("Graph is not fully connected, spectral embedding may not work as expected.")
        E, lam, res, n_iter = spectral_embedding(h, k, seed)
        t = dict(h.timings)
    t1 = time.perf_counter()
    km = kmeans(E, k, n_init=n_init, max_iter=SPECTRAL_KMEANS_MAX_ITER, device=device, rs=rs)
    t2 = time.perf_counter()
    return SpectralResult(km.labels, E, lam, res, n_iter, n_isolated,
                          {"affinity_ms": aff_ms, "normalise_ms": norm_ms, "products_ms": t["product_ms"],
                           "products_wall_ms": t["product_wall_ms"], "host_ms": t["host_ms"], "embedding_ms": 1e3 * (t1 - t0),
                           "kmeans_ms": 1e3 * (t2 - t1)})


# ------------------------------------------------------------------------------------------------ SKL-TSNE
# TSNE(n_components=dims, perplexity, early_exaggeration=4.0, learning_rate=1000.0, n_iter=1000, n_iter_without_progress=30,
#      min_grad_norm=1e-07, metric='euclidean', init, random_state=None, method, angle=0.5) (L1606-1621)
SKLTSNE_MAX_N = 50000                   # the dense n x n affinities of the exact method: 20 GB at the cap
SKLTSNE_MAX_ITER, SKLTSNE_EXPLORATION = 1000, 250       # max_iter; TSNE._EXPLORATION_MAX_ITER (stage 1, and its n_iter_without_progress)
SKLTSNE_N_ITER_CHECK, SKLTSNE_N_ITER_WITHOUT_PROGRESS, SKLTSNE_MIN_GRAD_NORM = 50, 30, 1e-7
SKLTSNE_EXAGGERATION = 4.0
SKLTSNE_METHODS = ("exact", "barnes_hut")       # the C ABI's method numbers
SKLTSNE_INITS = ("random", "pca")


class SKLTSNE(_Handle):
    """sklearn's TSNE on the GPU (frisk_skltsne_*): X (n x f, any f), the affinities and the float32 state (Y, update, gains) stay
    on the device.  method 'exact': dense joint probabilities; 'barnes_hut': the k = min(n - 1, int(3 perplexity + 1)) nearest
    neighbours of each row, whose conditionals the caller symmetrises (skl_tsne_joint_nn) and hands back with set_p().  Y starts at
    0; set the start with set().  Use as a context manager (or call close())."""

    _destroy = "frisk_skltsne_destroy"

    def __init__(self, X, dims=2, perplexity=20.0, method="barnes_hut", device=0):
        X = _f64(X, 2)
        self.n, self.f = X.shape
        self.dims, self.method = int(dims), method
        self.k = min(self.n - 1, int(3.0 * perplexity + 1))
        self._h = C.c_void_p()
        _call("frisk_skltsne_create", device, _ptr(X), self.n, self.f, float(perplexity), self.dims, SKLTSNE_METHODS.index(method),
              C.byref(self._h))

    def affinities(self):
        """(beta, steps) of every row: the beta its probabilities belong to and the bisection step that met the tolerance (100:
        none).  Computed once."""
        beta, steps = np.empty(self.n), np.empty(self.n, dtype=np.int32)
        _call("frisk_skltsne_affinities", self._h, _ptr(beta), _ptr(steps))
        return beta, steps

    def p_dense(self):
        """exact: the n x n joint P = max((C + CT) / max(sum, eps), eps), 0 on the diagonal."""
        P = np.empty((self.n, self.n))
        _call("frisk_skltsne_p_dense", self._h, _ptr(P))
        return P

    def neighbours(self):
        """barnes_hut: (indices n x k int32 in ascending column order, conditional p_j|i n x k)."""
        idx, cond = np.empty((self.n, self.k), dtype=np.int32), np.empty((self.n, self.k))
        _call("frisk_skltsne_neighbours", self._h, _ptr(idx), _ptr(cond))
        return idx, cond

    def set_p(self, P):
        """barnes_hut: the joint probabilities as a scipy CSR matrix (n x n); the values go up as float32, as sklearn passes them."""
        P = P.tocsr()
        if P.shape != (self.n, self.n):
            raise ValueError("expected a %d x %d matrix, got %s" % (self.n, self.n, P.shape))
        indptr = np.ascontiguousarray(P.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(P.indices, dtype=np.int32)
        values = np.ascontiguousarray(P.data, dtype=np.float32)
        _call("frisk_skltsne_set_p", self._h, _ptr(indptr), _ptr(indices), _ptr(values), int(values.size))

    def get(self):
        """(Y, update, gains), each n x dims float32."""
        out = [np.empty((self.n, self.dims), dtype=np.float32) for _ in range(3)]
        _call("frisk_skltsne_get", self._h, *[_ptr(a) for a in out])
        return tuple(out)

    def set(self, Y=None, update=None, gains=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (Y, update, gains)]
        for a in arrs:
            if a is not None and a.shape != (self.n, self.dims):
                raise ValueError("expected shape %s, got %s" % ((self.n, self.dims), a.shape))
        _call("frisk_skltsne_set", self._h, *[None if a is None else _ptr(a) for a in arrs])

    def run(self, begin, end, momentum, exaggeration=1.0):
        """Iterations begin .. end - 1 with P x exaggeration: (KL divergence, |grad * gains|) of the last of them."""
        err, norm = C.c_double(), C.c_double()
        _call("frisk_skltsne_run", self._h, int(begin), int(end), float(momentum), float(exaggeration), C.byref(err), C.byref(norm))
        return err.value, norm.value

    def last_ms(self):
        """Device ms: (the affinities, the last run)."""
        ms = _ffi.lib().frisk_skltsne_last_ms
        return ms(self._h, 0), ms(self._h, 1)


def skl_tsne_joint_nn(indices, cond):
    """sklearn's _joint_probabilities_nn from the conditionals of the kept neighbours (n x k each, columns ascending): P + PT on the
    union of the two patterns, divided by max(sum, eps).  A scipy CSR matrix (float64) with sorted column indices; n k entries is
    small, so this is the host's."""
    from scipy.sparse import csr_matrix
    n, k = indices.shape
    P = csr_matrix((np.asarray(cond, dtype=np.float64).ravel(), np.asarray(indices).ravel(), np.arange(0, n * k + 1, k)), shape=(n, n))
    P = P + P.T
    P /= np.maximum(P.sum(), np.finfo(np.double).eps)
    P = P.tocsr()
    P.sort_indices()
    return P


def skl_tsne_descent(h, max_iter=SKLTSNE_MAX_ITER, exploration=SKLTSNE_EXPLORATION, n_iter_check=SKLTSNE_N_ITER_CHECK,
                     n_iter_without_progress=SKLTSNE_N_ITER_WITHOUT_PROGRESS, min_grad_norm=SKLTSNE_MIN_GRAD_NORM,
                     exaggeration=SKLTSNE_EXAGGERATION):
    """The control flow of sklearn's TSNE._tsne and _gradient_descent on a handle h whose run(begin, end, momentum, exaggeration)
    performs iterations and returns (error, grad norm) of the last: stage 1 runs iterations 0 .. exploration - 1 with momentum 0.5
    and P x exaggeration (its n_iter_without_progress is `exploration`), stage 2 from the iteration after stage 1's last up to
    max_iter with momentum 0.8 and P as it is.  Every n_iter_check iterations the error and the norm are read: the stage stops when
    the error did not improve and i - best_iter > n_iter_without_progress, or when the norm is <= min_grad_norm; best_error restarts
    with each stage.  Returns (kl_divergence, n_iter, checks): the error of the last iteration run, its number (sklearn's n_iter_),
    and (iteration, error, norm) of every check."""
    checks = []

    def stage(it, stop_at, momentum, ex, patience):
        error = best_error = np.finfo(float).max
        best_iter = i = it
        nxt = it
        while nxt < stop_at:
            last = min(nxt + (n_iter_check - 1 - nxt % n_iter_check), stop_at - 1)     # the next check, or the last iteration
            error, norm = h.run(nxt, last + 1, momentum, ex)
            i = last
            if (i + 1) % n_iter_check == 0:
                checks.append((i, error, norm))
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > patience:
                    break
                if norm <= min_grad_norm:
                    break
            nxt = last + 1
        return error, i

    kl, it = stage(0, exploration, 0.5, exaggeration, exploration)
    if it < exploration or max_iter - exploration > 0:
        kl, it = stage(it + 1, max_iter, 0.8, 1.0, n_iter_without_progress)
    return kl, it, checks


class SKLTSNEResult:
    """Y (n x dims float32), kl_divergence and n_iter (sklearn's kl_divergence_ and n_iter_), errors and grad_norms (of every check,
    with check_iters their iterations), beta and steps of the perplexity search (n each), Y0 (the start); timings in ms."""

    def __init__(self, Y, kl_divergence, n_iter, checks, beta, steps, Y0, timings):
        self.Y, self.kl_divergence, self.n_iter = Y, kl_divergence, n_iter
        self.check_iters = np.array([c[0] for c in checks], dtype=np.int64)
        self.errors = np.array([c[1] for c in checks])
        self.grad_norms = np.array([c[2] for c in checks])
        self.beta, self.steps, self.Y0, self.timings = beta, steps, Y0, timings


def skl_tsne_check(n, f, dims, perplexity, method, init):
    """The argument errors of skl_tsne, sklearn's where it has one, raised before any device call."""
    if method not in SKLTSNE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (SKLTSNE_METHODS, method))
    if init not in SKLTSNE_INITS:
        raise ValueError("init must be one of %s, got %r" % (SKLTSNE_INITS, init))
    if not 2 <= n <= SKLTSNE_MAX_N:
        raise ValueError("SKL-TSNE needs between 2 and %d samples, got %d" % (SKLTSNE_MAX_N, n))
    if not perplexity > 0:
        raise ValueError("perplexity must be positive, got %r" % (perplexity,))
    if perplexity >= n:
        raise ValueError("perplexity must be less than n_samples")
    if dims < 1:
        raise ValueError("n_components=%d must be at least 1" % dims)
    if method == "barnes_hut" and dims > 3:
        raise ValueError("'n_components' should be inferior to 4 for the barnes_hut algorithm as it relies on quad-tree or oct-tree.")
    if dims > 64:
        raise ValueError("n_components=%d must be at most 64" % dims)
    if init == "pca" and dims > min(n, f):
        raise ValueError("n_components=%d must be between 1 and min(n_samples, n_features)=%d with init='pca'" % (dims, min(n, f)))


def skl_tsne_start(X, dims, rs, init="random", device=0):
    """The start of the embedding, float32: 'random' is sklearn's 1e-4 * rs.standard_normal((n, dims)).astype(float32); 'pca' is the
    exact PCA of this module (pca(): covariance and transform on the GPU, the same svd_flip sign rule) where sklearn runs
    PCA(svd_solver='randomized') from the same random state, then sklearn's cast to float32, division by std(column 0) and scaling
    by 1e-4.  The two PCAs agree up to the randomized solver's approximation error."""
    n = X.shape[0]
    if init == "pca":
        Y0 = pca(X, dims, device).Y.astype(np.float32, copy=False)
        return np.ascontiguousarray(Y0 / np.std(Y0[:, 0]) * 1e-4, dtype=np.float32)
    return np.ascontiguousarray(1e-4 * rs.standard_normal(size=(n, dims)).astype(np.float32), dtype=np.float32)


def skl_tsne(X, dims=2, perplexity=20.0, seed=0, method="barnes_hut", init="random", device=0):
    """sklearn 1.7's TSNE(n_components=dims, perplexity, early_exaggeration=4.0, learning_rate=1000.0, max_iter=1000,
    n_iter_without_progress=30, min_grad_norm=1e-07, metric='euclidean', init, random_state=seed, method, angle=0.5)
    .fit_transform(X) (L1606-1621; the reference's random_state=None becomes RandomState(seed)) on the GPU.  Affinities, every
    gradient and every update are kernels on a float32 state that stays on the device; the stop rule (skl_tsne_descent) reads two
    scalars every 50 iterations, so the run usually ends long before iteration 1000, as sklearn's does.
    Two departures from sklearn, both deliberate: (1) method='barnes_hut' keeps sklearn's sparse affinities (k nearest neighbours)
    but sums the repulsive term over ALL pairs instead of walking a quad-/oct-tree at angle = 0.5; that is what sklearn's own code
    computes as angle -> 0, so the result is sklearn's angle = 0 limit, not its angle = 0.5 approximation (which deviates from it by
    0.2 - 0.6 % of the largest gradient entry).  (2) init='pca' starts from this module's exact pca() instead of sklearn's
    randomized PCA (skl_tsne_start).  The trajectory is chaotic: the result matches sklearn's step by step and in its KL divergence
    and stopping iteration, not in its final coordinates.  Raises ValueError, before any device call, for sklearn's argument errors
    (perplexity >= n_samples; dims >= 4 with barnes_hut) and for n outside 2 .. 50 000."""
    X = _f64(X, 2)
    n, f = X.shape
    dims = int(dims)
    skl_tsne_check(n, f, dims, perplexity, method, init)
    rs = np.random.RandomState(seed)
    t0 = time.perf_counter()
    with SKLTSNE(X, dims, perplexity, method, device) as h:
        beta, steps = h.affinities()
        if method == "barnes_hut":
            h.set_p(skl_tsne_joint_nn(*h.neighbours()))
        t1 = time.perf_counter()
        Y0 = skl_tsne_start(X, dims, rs, init, device)
        t2 = time.perf_counter()
        h.set(Y=Y0)
        kl, n_iter, checks = skl_tsne_descent(h)
        Y = h.get()[0]
        t3 = time.perf_counter()
        aff_ms = h.last_ms()[0]
    return SKLTSNEResult(Y, kl, n_iter, checks, beta, steps, Y0,
                         {"affinities_ms": 1e3 * (t1 - t0), "affinities_device_ms": aff_ms, "init_ms": 1e3 * (t2 - t1),
                          "iterations_ms": 1e3 * (t3 - t2)})
