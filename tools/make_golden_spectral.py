#!/usr/bin/env python3
"""Goldens of spectral clustering (sklearn.cluster.SpectralClustering(n_clusters=k, eigen_solver=None, n_init=20, gamma=1.0,
affinity='rbf', eigen_tol=0.0, assign_labels='kmeans'), called at frisk/__init__.py L1659-1662 as .fit_predict(Y)):
tests/golden/spectral.json and .npy files under tests/golden/spectral/.  sklearn 1.7, scipy 1.15; the reference passes
random_state=None, the goldens a seed.  sklearn, scipy and numpy only: neither the package under test nor the reference is used.

Per case: Y, k, seed; sklearn's affinity_matrix_ (stored for n <= 200 only: an n x n array of doubles does not compress, and no
committed file may pass 1 MiB), scipy's dd, sklearn.manifold.spectral_embedding(affinity_matrix_, n_components=k, random_state=
RandomState(seed), drop_first=False, eigen_tol=0.0), the labels, and kpp: the indices sklearn.cluster.kmeans_plusplus picks on that
embedding from a RandomState(seed) that has spent the n draws of ARPACK's start vector (k_means' first seeding); from a full
numpy.linalg.eigh of the host M = (A0 / dd) / dd[:, None] symmetrised (A0 from direct differences, numpy's double), the top k + 1 eigenvalues and gap_k = lambda_k -
lambda_{k+1}; the number of isolated points (zero column sums).
Asserted per case, and a case that breaks one is not written:
  * gap_k >= 0.1;
  * sklearn's labels are the same partition for seed and seed + 3.
The cases are the smallest shapes at which the kernels can still go wrong: every tile edge of the affinity kernel (64), the column
blocks of the degrees (256) and its row ranges (32 rows at least, 256 ranges at most: n <= 700 stays below the cap), d = 1, 3, 5,
k = 1 .. 16, p = n, duplicates, an isolated point and an eigenvalue near -1.

    python tools/make_golden_spectral.py
"""
import json
import os
import sys
import warnings

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run
import numpy as np  # noqa: E402
from scipy.sparse import csgraph  # noqa: E402
from sklearn.cluster import SpectralClustering, kmeans_plusplus  # noqa: E402
from sklearn.manifold import spectral_embedding  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "..", "tests", "golden")
ARR = os.path.join(GOLD, "spectral")
MIN_GAP = 0.1
STORE_AFFINITY_UP_TO = 200


def blobs(seed, sizes, d, spread=0.25, step=5.0):
    """Gaussian blobs of the given sizes, spread `spread`, their centres `step` apart along a zigzag in the first two dims (one
    dim: along the line)."""
    rs = np.random.RandomState(seed)
    out = []
    for b, m in enumerate(sizes):
        centre = np.zeros(d)
        centre[0] = step * b
        if d > 1:
            centre[1] = step * (b % 2) * 0.5
        out.append(centre + spread * rs.normal(size=(m, d)))
    return np.vstack(out)


def build(name):
    if name == "blobs2":
        return blobs(1, (64, 65), 2), 2                         # n = 129: two tiles + 1
    if name == "blobs3":
        return blobs(2, (90, 70, 37), 2), 3                     # n = 197: three tiles + 5
    if name == "blobs5":
        return blobs(3, (40, 50, 30, 45, 32), 2), 5             # n = 197; the top eigenvalues agree to 1e-7
    if name == "d3":
        return blobs(4, (20, 25, 18), 3), 3                     # n = 63: tile - 1
    if name == "d1":
        return blobs(5, (30, 34), 1), 2                         # n = 64: one tile
    if name == "d5":
        return blobs(6, (20, 22, 23), 5), 3                     # n = 65: tile + 1
    if name == "k16":
        return blobs(7, (16,) * 16, 2, spread=0.2), 16          # n = 256: p = 26, the widest product
    if name == "p_eq_n":
        return blobs(8, (4, 5, 3), 2), 3                        # n = 12: p = n
    if name == "n2":
        return np.array([[0.0, 0.0], [0.5, 0.25]]), 1
    if name == "duplicates":
        Y = blobs(9, (30, 36), 2)
        Y[5] = Y[4]; Y[40] = Y[4 + 30]; Y[41] = Y[40]           # exact duplicates, within and across the tile's rows
        return Y, 2
    if name == "isolated":
        Y = blobs(10, (30, 35), 2)
        return np.vstack([Y, [[150.0, -150.0]]]), 2            # every affinity of the last point underflows to 0: w == 0 -> 1
    if name == "minus_one":
        Y = blobs(11, (30, 33), 2)
        return np.vstack([Y, [[2.5, 9.0], [2.5, 9.001]]]), 3    # two tight points far from the rest: eigenvalues +-1
    if name == "close3":
        return blobs(16, (60, 50, 40), 2, spread=0.5, step=2.6), 3     # blobs that touch: a small gap, the slowest iteration here
    if name == "n255":
        return blobs(12, (128, 127), 2), 2
    if name == "n257":
        return blobs(13, (100, 157), 2), 2
    if name == "n517":
        return blobs(14, (200, 150, 167), 2), 3                 # two column blocks of 256 + 5; 17 row ranges of 31 rows
    if name == "n645":
        return blobs(15, (300, 345), 2), 2                      # ten tiles + 5
    raise KeyError(name)


CASES = ["blobs2", "blobs3", "blobs5", "d3", "d1", "d5", "k16", "p_eq_n", "n2", "duplicates", "isolated", "minus_one", "n255",
         "n257", "n517", "n645", "close3"]


def partition(labels):
    seen = {}
    return [seen.setdefault(int(c), len(seen)) for c in labels]


def run(name, seed):
    Y, k = build(name)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n = Y.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # "Graph is not fully connected" where the case means it
        fits = [SpectralClustering(n_clusters=k, eigen_solver=None, random_state=s, n_init=20, gamma=1.0, affinity="rbf",
                                   eigen_tol=0.0, assign_labels="kmeans").fit(Y) for s in (seed, seed + 3)]
        A = fits[0].affinity_matrix_
        E = spectral_embedding(A, n_components=k, random_state=np.random.RandomState(seed), drop_first=False, eigen_tol=0.0)
    rs = np.random.RandomState(seed)
    rs.uniform(-1, 1, n)                                        # ARPACK's v0, as spectral_embedding draws it from the shared state
    kpp = kmeans_plusplus(E, k, random_state=rs)[1]             # the first seeding k_means then draws from the same state
    assert partition(fits[0].labels_) == partition(fits[1].labels_), "%s: sklearn's partition depends on the seed" % name
    A0 = A.copy()
    np.fill_diagonal(A0, 0.0)
    _lap, dd = csgraph.laplacian(A, normed=True, return_diag=True)
    iso = int(np.sum(A0.sum(axis=0) == 0))
    # the host M of the scheme itself: affinities from direct differences (sklearn's |x|^2 - 2 x.y + |y|^2 cancels, an error of a
    # few eps64 |x|^2 on the exponent that the eigenvalues would inherit), scipy's normalisation, symmetrised
    D = np.zeros((n, n))
    for c in range(Y.shape[1]):
        D += (Y[:, None, c] - Y[None, :, c]) ** 2
    H = np.exp(-1.0 * D)
    np.fill_diagonal(H, 0.0)
    w = H.sum(axis=0)
    assert int(np.sum(w == 0)) == iso, name
    hd = np.sqrt(np.where(w == 0, 1.0, w))
    M = (H / hd) / hd[:, None]
    lam = np.linalg.eigh(0.5 * (M + M.T))[0][::-1]
    top = lam[:k + 1]
    gap = float(top[k - 1] - top[k])
    assert gap >= MIN_GAP, "%s: gap_k = %g" % (name, gap)
    arrays = {"Y": Y, "dd": dd, "embedding": np.ascontiguousarray(E), "labels": np.asarray(partition(fits[0].labels_), dtype=np.int32),
              "kpp": np.asarray(kpp, dtype=np.int64)}
    if n <= STORE_AFFINITY_UP_TO:
        arrays["affinity"] = A
    for key, val in arrays.items():
        np.save(os.path.join(ARR, "%s.%s.npy" % (name, key)), val)
    return {"n": n, "d": int(Y.shape[1]), "k": k, "seed": seed, "gamma": 1.0, "n_isolated": iso, "top_eigenvalues": top.tolist(),
            "lambda_min": float(lam[-1]), "gap_k": gap, "arrays": sorted(arrays)}


def main():
    import scipy
    import sklearn
    os.makedirs(ARR, exist_ok=True)
    doc = {"sklearn": sklearn.__version__, "scipy": scipy.__version__, "numpy": np.__version__, "min_gap": MIN_GAP, "cases": {}}
    for i, name in enumerate(CASES):
        doc["cases"][name] = run(name, seed=i)
        c = doc["cases"][name]
        print("%-10s n %4d d %d k %2d  gap %.3f  lambda_min %+.4f  isolated %d" % (name, c["n"], c["d"], c["k"], c["gap_k"],
                                                                                  c["lambda_min"], c["n_isolated"]))
    with open(os.path.join(GOLD, "spectral.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    sys.exit(main())
