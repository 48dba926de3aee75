"""The projection and clustering kernels (csrc/proj_kernels.h) at their instantiation, tile and padding edges, against plain
high-precision oracles (tests/proj_oracles.py) and the edge goldens of tools/make_golden_projection.py:

    covariance and mean   f across the 16- and 64-column tile edges, n across the 16-row padding and the K split, n < f and
                          n >> f at F = 2 772, every entry held to its own forward error bound
    transform             f across the 64-lane stride, d up to 64
    PCA                   F = 2 772 against sklearn, tolerances scaled by the recorded eigengap
    DBSCAN                every db_pairs<MAXD> instantiation (MAXD = 4, 16, 64) at n on each LDS tile and block edge
    k-means               every km_assign<MAXD> instantiation, sklearn's empty-cluster relocation, explicit-init goldens
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import proj_oracles as PO
from golden_util import GOLD

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "projection_cluster.json")))
F = sum(PO.KMER_BLOCKS)


def A(name):
    return np.load(os.path.join(GOLD, "projection_cluster", name))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ covariance
def _data(n, f, seed):
    """proportion-like data with a non-zero mean; the k-mer layout at F = 2 772"""
    if f == F:
        return PO.kmer_like(n, seed)
    rs = np.random.RandomState(seed)
    X = rs.gamma(0.5, size=(n, f)) * (1.0 + 3.0 * rs.uniform(size=f))
    return X / X.sum(axis=1, keepdims=True) + 0.01 if f > 1 else X + 0.5


COV_SHAPES = [(1, 1), (2, 1), (17, 1), (3000, 1), (2, 15), (15, 15), (16, 63), (15, 64), (17, 65), (40, 63), (16, 64), (40, 65),
              (300, 128), (17, 128), (300, 692), (50001, 65), (50001, 692), (1, F), (2, F), (15, F), (16, F), (17, F), (40, F),
              (300, F), (3000, F), (20000, F)]


@pytest.mark.parametrize("n,f", COV_SHAPES)
def test_covariance_per_entry_against_longdouble(n, f):
    """frisk_proj_cov against the np.longdouble two-pass oracle, every entry within its own bound (PO.cov_oracle); at f = 2 772
    on the columns of every 16-column tile edge (every 64-column edge at n = 20 000), all pairs among them.  Exact symmetry,
    n = 1 divides by 1 (a zero matrix, no NaN), and a repeat call is bit-identical."""
    from frisk_amd.projection import cov
    X = _data(n, f, seed=n * 7 + f)
    m, c = cov(X)
    assert np.array_equal(c, c.T)
    cols = np.arange(f) if f <= 128 else PO.tile_edge_columns(f, 64 if n * f > 10 ** 7 else 16)
    mean, want, tol = PO.cov_oracle(X, cols)
    dm = PO.gamma(n + 1) * np.abs(X).sum(axis=0) / n
    assert np.all(np.abs(m - mean) <= 2 * dm + PO.U * np.abs(mean))
    got = c[np.ix_(cols, cols)]
    err = np.abs(got - np.asarray(want, dtype=np.float64))
    bad = np.argwhere(err > tol)
    assert bad.size == 0, "cov[%d][%d] off by %.3g, bound %.3g" % (cols[bad[0][0]], cols[bad[0][1]], err[tuple(bad[0])],
                                                                   tol[tuple(bad[0])])
    if n == 1:
        assert np.all(c == 0.0) and np.array_equal(m, X[0])
    if n in (17, 3000):
        m2, c2 = cov(X)
        assert m2.tobytes() == m.tobytes() and c2.tobytes() == c.tobytes()


@pytest.mark.parametrize("f,d", [(1, 1), (63, 1), (63, 17), (64, 2), (64, 64), (65, 2), (65, 64), (F, 1), (F, 2), (F, 17), (F, 64)])
def test_transform_per_entry_against_longdouble(f, d):
    from frisk_amd.projection import transform
    n = 301
    X = _data(n, f, seed=f + d)
    mean = X.mean(axis=0)
    V = np.random.RandomState(d).normal(size=(f, d))
    Y = transform(X, mean, V)
    want, tol = PO.transform_oracle(X, mean, V)
    assert np.all(np.abs(Y - np.asarray(want, dtype=np.float64)) <= tol)
    assert transform(X, mean, V).tobytes() == Y.tobytes()


@pytest.mark.parametrize("case", sorted(G["pca_large"]))
def test_pca_at_cli_feature_count_matches_sklearn(case):
    """PCA at F = 2 772 (the default --pcaMin 1 --pcaMax 6) against sklearn's full SVD.  Components compared after aligning
    signs (the sign rule itself is checked on ours), tolerances divided by the relative eigengap of the top d components."""
    from frisk_amd.projection import pca
    g = G["pca_large"][case]
    X = PO.planted_pca_input(g["n"], g["d"], g["seed"])
    assert X.shape == (g["n"], g["f"]) and PO.sha256(X) == g["sha256"]
    r = pca(X, g["d"])
    comps, Yg, ev = A(g["components"]), A(g["Y"]), A(g["explained_variance"])
    big = np.argmax(np.abs(r.components), axis=1)
    assert np.all(r.components[np.arange(g["d"]), big] > 0)
    s = np.sign(np.sum(r.components * comps, axis=1))
    tol = 1e-11 / g["eigengap"]
    assert np.abs(r.components * s[:, None] - comps).max() <= tol
    assert np.abs(r.Y * s[None, :] - Yg).max() <= tol * np.abs(Yg).max()
    assert np.abs(r.explained_variance - ev).max() <= 1e-10 * ev[0]
    assert np.abs(r.mean - X.mean(axis=0)).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ DBSCAN
@pytest.mark.parametrize("case", sorted(G["dbscan_edges"]))
def test_dbscan_matches_integer_goldens(case):
    """d = 5, 16, 17, 64 on integer coordinates: ties at exactly eps (3-4-5, 1-2-2-3), a border point two clusters reach, noise."""
    from frisk_amd.projection import dbscan
    g = G["dbscan_edges"][case]
    assert dbscan(A(g["Y"]), g["eps"], g["min_samples"]).tolist() == A(g["labels"]).tolist()


def _tile(d):
    return 4096 // (4 if d <= 4 else 16 if d <= 16 else 64)        # TP of db_pairs<MAXD> for this d


def _blobs(n, d, seed):
    rs = np.random.RandomState(seed)
    centres = rs.uniform(-6.0, 6.0, size=(5, d))
    Y = centres[rs.randint(0, 5, size=n)] + rs.normal(0.0, 1.0, size=(n, d))
    return Y


def _eps_for(Y, want_nb, rs):
    """eps giving about want_nb neighbours per point: the midpoint of two neighbouring distances of a sample, away from both"""
    i = rs.randint(0, len(Y), size=min(len(Y), 200))
    dist = np.unique(np.sqrt(((Y[i][:, None, :] - Y[None, :, :]) ** 2).sum(-1)))
    j = min(len(dist) - 2, int(len(dist) * want_nb / len(Y)))
    return float((dist[j] + dist[j + 1]) / 2)


@pytest.mark.parametrize("d", [2, 4, 5, 16, 17, 64])
@pytest.mark.parametrize("edge", ["1", "2", "255", "256", "257", "TP-1", "TP", "TP+1", "2TP+1"])
def test_dbscan_tile_and_block_edges_against_bruteforce(d, edge):
    """n on every tile edge (TP = 4096 / MAXD points per LDS tile: 1024, 256 or 64) and block edge (256 points), min_samples
    1, 2, 50 and n + 1, against the brute-force oracle; no pair lies within a relative 1e-9 of eps."""
    from frisk_amd.projection import dbscan
    tp = _tile(d)
    n = {"TP-1": tp - 1, "TP": tp, "TP+1": tp + 1, "2TP+1": 2 * tp + 1}.get(edge) or int(edge)
    rs = np.random.RandomState(n * 100 + d)
    Y = _blobs(n, d, n + d)
    eps = _eps_for(Y, 20, rs) if n > 2 else 1.0
    I, J, gap = PO.neighbour_pairs(Y, eps)
    assert gap > 1e-9
    for ms in (1, 2, 50, n + 1):
        got = dbscan(Y, eps, ms)
        want = PO.dbscan_labels(n, I, J, ms)
        assert np.array_equal(got, want), "min_samples %d" % ms
    if n > 50:
        assert (PO.dbscan_labels(n, I, J, 2) >= 0).any()


@pytest.mark.parametrize("d,n", [(5, 20000), (16, 16001), (17, 20000), (64, 8000)])
def test_dbscan_at_size_every_instantiation(d, n):
    from frisk_amd.projection import dbscan
    rs = np.random.RandomState(d)
    Y = _blobs(n, d, 50 + d)
    Y[rs.permutation(n)[:n // 20]] = rs.uniform(-12, 12, size=(n // 20, d))         # scattered noise
    eps = _eps_for(Y, 60, rs)
    want, gap = PO.dbscan_oracle(Y, eps, 50)
    assert gap > 1e-9 and (want == -1).any() and want.max() >= 1
    got = dbscan(Y, eps, 50)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("d", [2, 16, 64])
def test_dbscan_single_cluster_under_union_contention(d):
    """eps above the diameter: every point is a core point of one cluster, and every one of the n (n - 1) / 2 unions goes
    through the CAS union-find at once."""
    from frisk_amd.projection import dbscan
    n = 20000
    Y = np.random.RandomState(d).uniform(size=(n, d))
    assert (dbscan(Y, 2.0 * np.sqrt(d), 50) == 0).all()


# ------------------------------------------------------------------------------------------------ k-means
def _kmeans_abi(Y, C0, max_iter, tol):
    from frisk_amd import _ffi
    n, d = Y.shape
    k = C0.shape[0]
    Y, C0 = np.ascontiguousarray(Y, dtype=np.float64), np.ascontiguousarray(C0, dtype=np.float64)
    lab, cen = np.empty(n, np.int32), np.empty((k, d))
    ine, it = C.c_double(), C.c_int32()
    rc = _ffi.lib().frisk_kmeans(0, _ptr(Y), n, d, k, _ptr(C0), max_iter, tol, _ptr(lab), _ptr(cen), C.byref(ine), C.byref(it))
    assert rc == _ffi.OK
    return lab, cen, ine.value, it.value


@pytest.mark.parametrize("case", sorted(G["kmeans_init"]))
def test_kmeans_from_explicit_centres_matches_sklearn(case):
    """KMeans(init=C0, n_init=1): clusters emptied mid-run and relocated to the farthest points, duplicates at fewer than k
    locations, d = 5, 17, 64, k = 1, k = n."""
    g = G["kmeans_init"][case]
    Y = A(g["Y"])
    lab, cen, inertia, it = _kmeans_abi(Y, A(g["init"]), g["max_iter"], g["tol"])
    want = A(g["centers"])
    assert lab.tolist() == A(g["labels"]).tolist()
    assert np.abs(cen - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert abs(inertia - g["inertia"]) <= 1e-12 * max(g["inertia"], 1.0)
    assert it == g["n_iter"]


@pytest.mark.parametrize("case", sorted(G["kmeans_more"]))
def test_kmeans_plusplus_matches_sklearn_at_higher_d(case):
    from frisk_amd.projection import kmeans
    g = G["kmeans_more"][case]
    Y = A(g["Y"])
    r = kmeans(Y, g["k"], seed=0)
    a, b = r.labels, A(g["labels"])
    assert len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist())) == g["k"]
    assert abs(r.inertia - g["inertia"]) <= 1e-9 * g["inertia"]


@pytest.mark.parametrize("d", [4, 5, 16, 17, 64])
@pytest.mark.parametrize("n", [255, 256, 257, 200000])
def test_kmeans_against_lloyd_restatement(n, d):
    """km_assign<MAXD> at every instantiation and n on the 256-point block edge, k = 1 and 9, one step (max_iter = 1) and tol = 0,
    against PO.lloyd.  Continuous data: labels exact (no near ties), centres and inertia to 1e-12."""
    rs = np.random.RandomState(n + d)
    Y = _blobs(n, d, 7 * d)
    for k, max_iter, tol in ((9, 1, 1e-4), (9, 30, 0.0), (1, 5, 0.0)):
        C0 = Y[rs.choice(n, k, replace=False)] + rs.normal(0.0, 0.1, size=(k, d))
        lab, cen, inertia, it = _kmeans_abi(Y, C0, max_iter, tol)
        wl, wc, wi, wit = PO.lloyd(Y, C0, max_iter, tol)
        assert np.array_equal(lab, wl), (k, max_iter)
        assert np.abs(cen - wc).max() <= 1e-12 * np.abs(wc).max() and abs(inertia - wi) <= 1e-12 * wi and it == wit


@pytest.mark.parametrize("d", [2, 5, 17, 64])
def test_kmeans_integer_ties_and_relocation_bit_exact(d):
    """Integer points and centres: sums are exact in any order, so the kernel and PO.lloyd agree to the bit through every step.
    Many points lie at equal distance from two centres (the lowest index wins), and three centres start far from every point,
    so they empty in the first step and take the three farthest points (ties among them broken by the lowest index)."""
    rs = np.random.RandomState(d)
    n, k = 3001, 8
    Y = rs.randint(0, 5, size=(n, d)).astype(np.float64)
    C0 = rs.randint(0, 5, size=(k, d)).astype(np.float64)
    C0[[1, 4, 6]] += 1000.0
    trace = []
    wl, wc, wi, wit = PO.lloyd(Y, C0, 100, 0.0, trace)
    assert trace[0]["empty"] >= 3 and len(trace[0]["moved"]) == trace[0]["empty"]
    lab, cen, inertia, it = _kmeans_abi(Y, C0, 100, 0.0)
    assert np.array_equal(lab, wl) and cen.tobytes() == wc.tobytes() and it == wit
    assert abs(inertia - wi) <= 1e-12 * wi


def test_kmeans_relocation_many_blocks():
    """Four clusters empty in one step at n = 100 000: the farthest points are picked across all blocks, in descending distance."""
    rs = np.random.RandomState(3)
    n, d = 100000, 5
    Y = _blobs(n, d, 11)
    C0 = Y[rs.choice(n, 9, replace=False)].copy()
    C0[[0, 3, 5, 8]] = 500.0 + rs.uniform(size=(4, d))
    trace = []
    wl, wc, wi, wit = PO.lloyd(Y, C0, 40, 0.0, trace)
    assert trace[0]["empty"] == 4 and trace[0]["unique_far"]
    lab, cen, inertia, it = _kmeans_abi(Y, C0, 40, 0.0)
    assert np.array_equal(lab, wl) and it == wit
    assert np.abs(cen - wc).max() <= 1e-12 * np.abs(wc).max() and abs(inertia - wi) <= 1e-12 * wi


def test_kmeans_renumbering_keeps_all_clusters_after_relocation():
    """projection.kmeans renumbers labels by first occurrence and drops centres nobody uses: with relocation every one of the k
    clusters is used unless the points sit at fewer than k locations."""
    from frisk_amd.projection import kmeans
    Y = _blobs(2000, 3, 5)
    r = kmeans(Y, 7, seed=1)
    assert sorted(set(r.labels.tolist())) == list(range(7)) and r.centers.shape == (7, 3)
    Y = np.repeat(np.array([[0.0, 0.0], [1.0, 2.0], [5.0, 5.0]]), 40, axis=0)
    r = kmeans(Y, 5, seed=1)
    assert sorted(set(r.labels.tolist())) == [0, 1, 2] and r.inertia == 0.0


# ------------------------------------------------------------------------------------------------ C ABI bounds
def test_abi_dimension_and_k_bounds():
    from frisk_amd import _ffi
    L = _ffi.lib()
    rs = np.random.RandomState(0)
    for d, ok in ((64, _ffi.OK), (65, _ffi.E_ARG)):
        Y = rs.uniform(size=(30, d))
        lab = np.empty(30, np.int32)
        assert L.frisk_dbscan(0, _ptr(Y), 30, d, 0.5, 3, _ptr(lab)) == ok
        cen = np.empty((3, d))
        ine, it = C.c_double(), C.c_int32()
        assert L.frisk_kmeans(0, _ptr(Y), 30, d, 3, _ptr(np.ascontiguousarray(Y[:3])), 10, 0.0, _ptr(lab), _ptr(cen),
                              C.byref(ine), C.byref(it)) == ok
    Y = rs.uniform(size=(30, 64))
    lab, cen = _kmeans_abi(Y, Y[::-1], 10, 0.0)[:2]                  # k = n: each point its own cluster
    assert lab.tolist() == list(range(29, -1, -1)) and np.array_equal(cen, Y[::-1])
