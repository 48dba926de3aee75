"""Plain numpy oracles of the projection and clustering kernels (csrc/proj_kernels.h), shared by the CPU and GPU tests and by
tools/make_golden_projection.py (which keeps a k-means golden only where lloyd() below agrees with sklearn).

    cov_oracle       covariance in np.longdouble with two-pass centring, on a subset of columns, and a per-entry forward error
                     bound of the FP64 kernel
    lloyd            the kernel's Lloyd iteration, sklearn's empty-cluster relocation included
    dbscan_oracle    brute-force DBSCAN in any dimension, squares summed in dimension order, labelled as sklearn's dbscan_inner
    kmer_like        row-normalised integer counts with the feature layout of --pcaMin 1 --pcaMax 6 (F = 2 772)
"""
import hashlib

import numpy as np

U = np.finfo(np.float64).eps / 2          # unit roundoff of FP64
KMER_BLOCKS = (2, 10, 32, 136, 512, 2080)  # features of orders 1..6 after scrubMirrors: 2 772 in all


# ------------------------------------------------------------------------------------------------ covariance
def tile_edge_columns(f, step=16):
    """0, f - 1 and both sides of every multiple of `step` below f: the columns where a mis-indexed MFMA sub-tile or a padding
    error shows first."""
    cols = {0, f - 1}
    for e in range(step, f, step):
        cols.update((e - 1, e))
    return np.array(sorted(c for c in cols if 0 <= c < f), dtype=np.int64)


def gamma(m):
    return m * U / (1.0 - m * U)


def cov_oracle(X, cols=None):
    """(mean, cov[cols][:, cols], tol[cols][:, cols]) for X (n x f, float64).

    The oracle is computed in np.longdouble with two-pass centring.  tol bounds the error of the kernel, which computes, in
    FP64 and in some fixed order,
      m_j  = (sum_r x_rj) / n                             |m_j - mean_j|  <= dm_j = gamma(n + 1) sum_r |x_rj| / n
      y_rj = fl(x_rj - m_j)                               |y_rj - xc_rj| <= e_rj = dm_j + U (|xc_rj| + dm_j)
      c_ij = fl(sum_r y_ri y_rj) / (n - 1)                any summation order: error <= gamma(n) sum_r |y_ri| |y_rj|
    With a_ij = (|Xc|T |Xc|)_ij and s_i = sum_r |xc_ri|, to first order in U
      |c_ij - cov_ij| (n - 1) <= gamma(n + 2) a_ij + dm_j s_i + dm_i s_j + n dm_i dm_j (+ U |cov_ij| (n - 1) for the division);
    tol is twice that, entry by entry, so a small-variance block (the k = 6 features) is held to its own scale and not to the
    largest entry of the matrix.  n = 1 divides by 1, as the kernel does."""
    X = np.asarray(X, dtype=np.float64)
    n, f = X.shape
    cols = np.arange(f) if cols is None else np.asarray(cols)
    mean = X.sum(axis=0, dtype=np.longdouble) / n
    XcL = X[:, cols].astype(np.longdouble) - mean[cols]
    denom = float(n - 1) if n > 1 else 1.0
    c = (XcL.T @ XcL) / denom
    Xc = np.asarray(XcL, dtype=np.float64)
    A = np.abs(Xc).T @ np.abs(Xc)
    s = np.abs(Xc).sum(axis=0)
    dm = gamma(n + 1) * np.abs(X[:, cols]).sum(axis=0) / n
    bound = gamma(n + 2) * A + np.outer(s, dm) + np.outer(dm, s) + n * np.outer(dm, dm)
    tol = 2.0 * (bound / denom + 2 * U * np.abs(np.asarray(c, dtype=np.float64)))
    return np.asarray(mean, dtype=np.float64), c, tol


def transform_oracle(X, mean, V):
    """(Y, tol) of (X - mean) V, Y in np.longdouble; tol from |fl(x - m) - (x - m)| <= U |x - m| and any summation order:
    2 (gamma(f + 1) |X - mean| |V|)."""
    XL = np.asarray(X, dtype=np.longdouble) - np.asarray(mean, dtype=np.longdouble)
    Y = XL @ np.asarray(V, dtype=np.longdouble)
    A = np.abs(np.asarray(XL, dtype=np.float64)) @ np.abs(V)
    return Y, 2.0 * gamma(X.shape[1] + 1) * A + 2 * U * np.abs(np.asarray(Y, dtype=np.float64))


def kmer_like(n, seed, depth=4000):
    """n rows of proportions with the feature layout of k-mer orders 1..6 (KMER_BLOCKS): each order's block is integer counts
    normalised to sum 1, so the variances of the order-6 features lie orders of magnitude below those of order 1."""
    rs = np.random.RandomState(seed)
    out = []
    for m in KMER_BLOCKS:
        p = rs.dirichlet(np.full(m, 2.0))
        lam = depth * p[None, :] * rs.gamma(4.0, 0.25, size=(n, m))
        cnt = rs.poisson(lam).astype(np.float64) + 1.0
        out.append(cnt / cnt.sum(axis=1, keepdims=True))
    return np.hstack(out)


def planted_pca_input(n, d, seed):
    """Row-normalised integer counts (F = 2 772, the layout of kmer_like) with d planted directions of well-separated variance
    above the rest, so that the top d components are well conditioned."""
    rs = np.random.RandomState(seed)
    f = sum(KMER_BLOCKS)
    base = rs.uniform(20.0, 60.0, size=f)
    dirs = rs.normal(size=(d, f))
    z = rs.normal(size=(n, d)) * np.array([12.0 * 0.6 ** t for t in range(d)])
    lam = base[None, :] * np.exp(0.25 * np.tanh(z @ dirs / 8.0))
    cnt = rs.poisson(lam).astype(np.float64)
    return cnt / cnt.sum(axis=1, keepdims=True)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ k-means
def sq_dist(Y, C):
    """n x k squared distances, squares summed in dimension order (as km_assign sums them)."""
    D = np.zeros((Y.shape[0], C.shape[0]))
    for q in range(Y.shape[1]):
        t = Y[:, q, None] - C[None, :, q]
        D += t * t
    return D


def lloyd_step(Y, C, trace=None):
    """One Lloyd step as km_assign + km_update: labels (nearest centre, lowest index on a tie), the new centres after sklearn's
    empty-cluster relocation and averaging, the squared centre shift, the inertia of the assignment."""
    n, d = Y.shape
    k = C.shape[0]
    D = sq_dist(Y, C)
    lab = np.argmin(D, axis=1)
    dist = D[np.arange(n), lab]
    S = np.zeros((k, d))
    np.add.at(S, lab, Y)
    W = np.bincount(lab, minlength=k).astype(np.float64)
    empty = np.flatnonzero(W == 0)
    moved = []
    if empty.size and dist.max() > 0:
        far = np.lexsort((np.arange(n), -dist))[:empty.size]     # descending distance, lowest index on a tie
        for nc, i in zip(empty, far):
            oc = lab[i]
            S[oc] -= Y[i]
            S[nc] = Y[i]
            W[nc] = 1.0
            W[oc] -= 1.0
            moved.append((int(nc), int(i)))
    if trace is not None:
        srt = np.sort(dist)[::-1]
        trace.append({"empty": int(empty.size), "moved": moved,
                      "unique_far": bool(empty.size == 0 or srt.size <= empty.size or srt[empty.size - 1] > srt[empty.size])})
    a = int(np.argmax(W))
    Cn = np.empty_like(C)
    for c in range(k):
        if W[c] > 0:
            Cn[c] = S[c] / W[c]
        else:
            Cn[c] = S[a] / W[a] if a < c else S[a]
    shift = float(np.sum((Cn - C) ** 2))
    return lab, Cn, shift, float(dist.sum())


def lloyd(Y, C0, max_iter, tol, trace=None):
    """frisk_kmeans restated: (labels, centres, inertia, n_iter).  Stops as sklearn's Lloyd does (labels unchanged, or squared
    centre shift <= tol, or max_iter steps), then assigns once more to the final centres."""
    Y = np.asarray(Y, dtype=np.float64)
    C = np.array(C0, dtype=np.float64)
    old = np.full(Y.shape[0], -1)
    it = 0
    for it in range(max_iter):
        lab, C, shift, _ = lloyd_step(Y, C, trace)
        if np.array_equal(lab, old) or shift <= tol:
            break
        old = lab
    D = sq_dist(Y, C)
    lab = np.argmin(D, axis=1)
    return lab.astype(np.int32), C, float(D[np.arange(len(lab)), lab].sum()), min(it + 1, max_iter)


# ------------------------------------------------------------------------------------------------ DBSCAN
def neighbour_pairs(Y, eps, chunk=256, max_pairs=60_000_000):
    """(I, J, gap): every ordered neighbour pair (sqrt(sum_k (y_ik - y_jk)^2) <= eps, squares summed in dimension order, as
    db_pairs sums them; i == j included), by brute force in row chunks; gap = min |dist - eps| / eps over all pairs, so that a
    caller can assert no decision was within rounding of eps."""
    Y = np.asarray(Y, dtype=np.float64)
    n, d = Y.shape
    I, J = [], []
    total, gap = 0, np.inf
    for i0 in range(0, n, chunk):
        B = Y[i0:i0 + chunk]
        s = np.zeros((B.shape[0], n))
        for q in range(d):
            t = B[:, q, None] - Y[None, :, q]
            s += t * t
        dist = np.sqrt(s)
        gap = min(gap, float(np.min(np.abs(dist - eps))) / eps)
        ii, jj = np.nonzero(dist <= eps)
        total += ii.size
        assert total <= max_pairs, "too many neighbour pairs for the oracle"
        I.append(ii + i0)
        J.append(jj)
    return np.concatenate(I), np.concatenate(J), gap


def dbscan_labels(n, I, J, min_samples):
    """sklearn's dbscan_inner labelling from the neighbour pairs: clusters = components of the core points, numbered in increasing
    order of their smallest index; a border point joins the first cluster (smallest root) among its core neighbours."""
    core = np.bincount(I, minlength=n) >= min_samples
    cc = core[I] & core[J]
    ci, cj = I[cc], J[cc]
    root = np.arange(n)
    while True:                       # min-label propagation with pointer jumping
        old = root.copy()
        np.minimum.at(root, ci, root[cj])
        root = root[root]
        if np.array_equal(root, old):
            break
    lab = np.full(n, -1, dtype=np.int64)
    lab[core] = root[core]
    border = ~core[I] & core[J]
    big = np.iinfo(np.int64).max
    best = np.full(n, big)
    np.minimum.at(best, I[border], root[J[border]])
    nb = ~core & (best < big)
    lab[nb] = best[nb]
    roots = np.unique(lab[lab >= 0])
    out = np.full(n, -1, dtype=np.int64)
    out[lab >= 0] = np.searchsorted(roots, lab[lab >= 0])
    return out


def dbscan_oracle(Y, eps, min_samples):
    """(labels, gap) of DBSCAN(eps, min_samples) on Y of any dimension."""
    I, J, gap = neighbour_pairs(Y, eps)
    return dbscan_labels(len(Y), I, J, min_samples), gap
