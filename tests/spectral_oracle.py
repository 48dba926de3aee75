"""sklearn 1.7's SpectralClustering(affinity='rbf', assign_labels='kmeans') restated in numpy for the tests, independently of
frisk_amd.projection: the rbf affinities by direct differences, scipy's csgraph.laplacian(normed=True) normalisation, the top k
eigenpairs of M = D^-1/2 A0 D^-1/2 by the block subspace iteration with Rayleigh-Ritz on M + I that frisk_amd.projection.
spectral_embedding drives on the GPU, sklearn's post-processing (divide by dd, _deterministic_vector_sign_flip, transpose), and a
plain Lloyd k-means from sklearn's greedy k-means++ seeds.  No sklearn import; the goldens (tests/golden/spectral.json,
tools/make_golden_spectral.py) are sklearn's own results.

What can be compared with sklearn.  ARPACK and the iteration here converge to the same invariant subspace of the top k
eigenvalues, but where eigenvalues (nearly) coincide - k well separated blobs give k eigenvalues within 1e-7 of 1 - the single
vectors are any rotation of each other.  So the comparisons are of the subspace (subspace_sine, bounded by Davis-Kahan:
sin(angle) <= (r_a + r_b) / gap_k for residual norms r and gap_k = lambda_k - lambda_{k+1}), of the embedding rows' pairwise
distances (invariant under a rotation of the columns), and of the labels as a partition."""
import json
import os

import numpy as np

EPS = np.finfo(np.float64).eps
TOL, MAX_ITER, GUARD = 1e-10, 500, 10
KMEANS_MAX_ITER, KMEANS_TOL = 300, 1e-4

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden():
    return json.load(open(os.path.join(GOLD, "spectral.json")))


def array(case, name):
    return np.load(os.path.join(GOLD, "spectral", "%s.%s.npy" % (case, name)))


# ------------------------------------------------------------------------------------------------ the matrix
def sqdist(Y, dtype=np.float64):
    """sum_c (y_ic - y_jc)^2, c in order, by direct differences."""
    Y = np.asarray(Y, dtype=dtype)
    s = np.zeros((Y.shape[0], Y.shape[0]), dtype=dtype)
    for c in range(Y.shape[1]):
        t = Y[:, None, c] - Y[None, :, c]
        s += t * t
    return s


def affinity(Y, gamma=1.0):
    A = np.exp(-gamma * sqdist(Y))
    np.fill_diagonal(A, 0.0)
    return A


def degrees(A):
    """(dd, number of columns whose sum was 0) as scipy's _laplacian_dense: w = column sums, w == 0 -> 1, dd = sqrt(w)."""
    w = A.sum(axis=0)
    iso = w == 0
    return np.sqrt(np.where(iso, 1.0, w)), int(iso.sum())


def scipy_matrix(A, dd):
    """scipy's two in-place divisions: m /= dd, then m /= dd[:, None].  Not exactly symmetric."""
    return (A / dd) / dd[:, None]


def matrix(A, dd):
    """The device's M: the mean of scipy's entry and its mirror (exactly symmetric, within 1 ulp of either)."""
    m = scipy_matrix(A, dd)
    return 0.5 * (m + m.T)


# ------------------------------------------------------------------------------------------------ the embedding
def sign_flip(E):
    """sklearn's _deterministic_vector_sign_flip on the rows of E."""
    big = np.argmax(np.abs(E), axis=1)
    return E * np.sign(E[np.arange(E.shape[0]), big])[:, None]


def embedding(M, dd, k, seed=0, tol=TOL, max_iter=MAX_ITER, mq=None):
    """(E n x k, eigenvalues of M, residuals, iterations); mq(Q) = M Q (default: numpy's matmul)."""
    n = M.shape[0]
    mq = mq or (lambda Q: M @ Q)
    p = min(k + GUARD, n)
    Q = np.linalg.qr(np.random.RandomState(seed).uniform(-1, 1, (n, p)))[0]
    for it in range(1, max_iter + 1):
        MQ = mq(Q)
        Z = MQ + Q
        B = Q.T @ Z
        theta, S = np.linalg.eigh(0.5 * (B + B.T))
        theta, S = theta[::-1], S[:, ::-1]
        ZS, V = Z @ S, Q @ S
        res = np.sqrt(np.sum((ZS - V * theta) ** 2, axis=0))[:k]
        if res.max() <= tol:
            break
        Q = np.linalg.qr(ZS)[0]
    lam = np.sum(V[:, :k] * (MQ @ S[:, :k]), axis=0) / np.sum(V[:, :k] * V[:, :k], axis=0)      # Rayleigh quotients against M
    E = sign_flip(V[:, :k].T / dd)
    return np.ascontiguousarray(E.T), lam, res, it


def orthonormal(E, dd):
    """An orthonormal basis of the span of the eigenvectors behind an embedding E (n x k): qr of dd o E."""
    return np.linalg.qr(E * dd[:, None])[0]


def residual(M, V):
    """The 2-norm of M V - V (VT M V) for orthonormal V: how far span(V) is from an invariant subspace of M."""
    MV = M @ V
    return float(np.linalg.norm(MV - V @ (V.T @ MV), 2))


def subspace_sine(V, Vg):
    """|(I - Vg VgT) V|_2 for orthonormal V, Vg: the sine of the largest angle between the two subspaces."""
    return float(np.linalg.norm(V - Vg @ (Vg.T @ V), 2))


def row_distances(E):
    return np.sqrt(sqdist(E))


# ------------------------------------------------------------------------------------------------ k-means
def kmeans_plusplus(X, k, rs):
    """sklearn's _kmeans_plusplus (2 + floor(ln k) local trials) with uniform weights, drawing from rs."""
    n = X.shape[0]
    trials = 2 + int(np.log(k))

    def d2(P):
        return np.maximum(((P[:, None, :] - X[None, :, :]) ** 2).sum(axis=2), 0.0)
    first = int(rs.choice(n, p=np.full(n, 1.0 / n)))
    idx = [first]
    closest = d2(X[[first]])[0]
    pot = closest.sum()
    for _ in range(1, k):
        r = rs.uniform(size=trials) * pot
        cand = np.minimum(np.searchsorted(np.cumsum(closest), r), n - 1)
        dc = np.minimum(closest, d2(X[cand]))
        pots = dc.sum(axis=1)
        b = int(np.argmin(pots))
        pot, closest = pots[b], dc[b]
        idx.append(int(cand[b]))
    return X[idx].copy()


def lloyd(X, centers, max_iter=KMEANS_MAX_ITER, tol=KMEANS_TOL):
    """Plain Lloyd from `centers`: (labels, inertia).  Stops when the centres move by at most tol * mean variance (sklearn's rule)
    or the labels repeat; an empty cluster keeps its centre."""
    tol_abs = float(np.mean(np.var(X, axis=0))) * tol
    labels = None
    for _ in range(max_iter):
        d = ((X[:, None, :] - centers[None, :, :]) ** 2).sum(axis=2)
        new = np.argmin(d, axis=1)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        moved = 0.0
        for c in range(centers.shape[0]):
            if np.any(labels == c):
                m = X[labels == c].mean(axis=0)
                moved += float(((m - centers[c]) ** 2).sum())
                centers[c] = m
        if moved <= tol_abs:
            break
    d = ((X[:, None, :] - centers[None, :, :]) ** 2).sum(axis=2)
    labels = np.argmin(d, axis=1)
    return labels, float(d[np.arange(X.shape[0]), labels].sum())


def kmeans(X, k, rs, n_init=20):
    best = None
    for _ in range(n_init):
        labels, inertia = lloyd(X, kmeans_plusplus(X, k, rs))
        if best is None or inertia < best[1]:
            best = (labels, inertia)
    return renumber(best[0])


def renumber(labels):
    """Cluster ids by first occurrence in row order."""
    seen, out = {}, np.empty(len(labels), dtype=np.int32)
    for i, c in enumerate(np.asarray(labels).tolist()):
        out[i] = seen.setdefault(c, len(seen))
    return out


def same_partition(a, b):
    return np.array_equal(renumber(a), renumber(b))


# ------------------------------------------------------------------------------------------------ the whole pipeline
def pipeline(Y, k, seed=0, gamma=1.0, n_init=20):
    """dict(A, dd, n_isolated, M, embedding, eigenvalues, residuals, n_iter, labels) of the whole scheme on the host."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    rs = np.random.RandomState(seed)
    rs.uniform(-1, 1, n)                        # the draws sklearn spends on ARPACK's v0
    A = affinity(Y, gamma)
    dd, iso = degrees(A)
    M = matrix(A, dd)
    E, lam, res, it = embedding(M, dd, k, seed)
    return {"A": A, "dd": dd, "n_isolated": iso, "M": M, "embedding": E, "eigenvalues": lam, "residuals": res, "n_iter": it,
            "labels": kmeans(E, k, rs, n_init)}


# ------------------------------------------------------------------------------------------------ shared checks
def host_matrix(case):
    """(A, dd, M) of the oracle: the scheme on the host, from direct differences (the golden's dd is scipy's from sklearn's
    affinities, which differ by the cancellation of |x|^2 - 2 x.y + |y|^2)."""
    A = affinity(array(case, "Y"), golden()["cases"][case]["gamma"])
    dd = degrees(A)[0]
    return A, dd, matrix(A, dd)


def check_embedding(case, E, lam, res, M, dd):
    """E against sklearn's: eigenvalues within residual + n eps64, the subspace within (r_ours + r_golden) / gap_k + n eps64
    (both residuals computed here from the host M), the rows' pairwise distances within that bound times 2 max(1 / dd)."""
    g = golden()["cases"][case]
    n, k = g["n"], g["k"]
    Eg = array(case, "embedding")
    assert E.shape == Eg.shape == (n, k)
    assert np.all(np.abs(lam - np.array(g["top_eigenvalues"][:k])) <= res.max() + n * EPS), case
    V, Vg = orthonormal(E, dd), orthonormal(Eg, array(case, "dd"))         # each with the dd it was divided by
    bound = (residual(M, V) + residual(M, Vg)) / g["gap_k"] + n * EPS
    sine = subspace_sine(V, Vg)
    assert sine <= bound, (case, sine, bound)
    gap = np.abs(row_distances(E) - row_distances(Eg)).max()
    assert gap <= bound * 2 * float((1.0 / dd).max()), (case, gap, bound)
    return sine / bound
