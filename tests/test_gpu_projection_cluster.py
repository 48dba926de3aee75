"""Projection and clustering on the GPU (csrc/proj_kernels.h through frisk_amd.projection): PCA, DBSCAN and k-means against
sklearn goldens and numpy oracles at larger sizes, run-to-run bit identity, argument checks of the C ABI, and the CLI end to end
writing the reference's cluster-labelled GFF3."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLD, INPUTS

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLD, "projection_cluster.json")))
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def A(name):
    """an array of the golden (tests/golden/projection_cluster/<name>)"""
    return np.load(os.path.join(GOLD, "projection_cluster", name))


# ------------------------------------------------------------------------------------------------ PCA
@pytest.mark.parametrize("case", sorted(G["pca"]))
def test_pca_matches_sklearn_golden(case):
    from frisk_amd.projection import pca
    g = G["pca"][case]
    X, Yg = A(g["X"]), A(g["Y"])
    r = pca(X, g["d"])
    scale = np.abs(Yg).max()
    assert np.abs(r.Y - Yg).max() <= 1e-9 * scale
    assert np.abs(r.components - A(g["components"])).max() <= 1e-9
    ev = A(g["explained_variance"])
    assert np.abs(r.explained_variance - ev).max() <= 1e-9 * ev.max()
    assert np.abs(r.mean - A(g["mean"])).max() <= 1e-12 * np.abs(X).max()


def _proportions(n, f, seed):
    rs = np.random.RandomState(seed)
    X = rs.gamma(0.5, size=(n, f)) * (1.0 + 3.0 * rs.uniform(size=f))
    return X / X.sum(axis=1, keepdims=True)


def test_covariance_and_transform_at_size_against_numpy():
    """n = 50 000, F = 692 (--pcaMax 5): covariance and transform against a float64 numpy oracle; two runs are bit-identical."""
    from frisk_amd.projection import cov, pca, transform
    n, f = 50000, 692
    X = _proportions(n, f, 1)
    mean = X.mean(axis=0)
    Xc = X - mean
    want = (Xc.T @ Xc) / (n - 1)
    m, c = cov(X)
    assert np.abs(m - mean).max() <= 1e-15
    assert np.array_equal(c, c.T)
    assert np.abs(c - want).max() <= 1e-9 * np.abs(want).max()
    V = np.linalg.qr(np.random.RandomState(2).normal(size=(f, 4)))[0]
    Y = transform(X, m, V)
    Yw = Xc @ V
    assert np.abs(Y - Yw).max() <= 1e-9 * np.abs(Yw).max()
    a, b = pca(X, 3), pca(X, 3)
    assert a.Y.tobytes() == b.Y.tobytes() and a.components.tobytes() == b.components.tobytes()
    m2, c2 = cov(X)
    assert c2.tobytes() == c.tobytes() and m2.tobytes() == m.tobytes()


# ------------------------------------------------------------------------------------------------ DBSCAN
@pytest.mark.parametrize("case", sorted(G["dbscan"]))
def test_dbscan_matches_sklearn_golden(case):
    from frisk_amd.projection import dbscan
    g = G["dbscan"][case]
    labels = dbscan(A(g["Y"]), g["eps"], G["min_samples"])
    assert labels.tolist() == A(g["labels"]).tolist()


def _dbscan_oracle(Y, eps, min_samples):
    """DBSCAN labels as sklearn's dbscan_inner numbers them, from grid buckets of side eps (numpy, d = 2)."""
    n = Y.shape[0]
    cell = np.floor(Y / eps).astype(np.int64)
    cell -= cell.min(axis=0)
    width = int(cell[:, 1].max()) + 3
    key = (cell[:, 0] + 1) * width + (cell[:, 1] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    I, J = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            nk = key + dx * width + dy
            lo, hi = np.searchsorted(skey, nk, "left"), np.searchsorted(skey, nk, "right")
            cnt = hi - lo
            i = np.repeat(np.arange(n), cnt)
            start = np.repeat(lo - np.concatenate(([0], np.cumsum(cnt)[:-1])), cnt)
            j = order[start + np.arange(i.size)]
            t0, t1 = Y[i, 0] - Y[j, 0], Y[i, 1] - Y[j, 1]
            ok = np.sqrt(t0 * t0 + t1 * t1) <= eps
            I.append(i[ok]); J.append(j[ok])
    I, J = np.concatenate(I), np.concatenate(J)
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
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, I[border], root[J[border]])
    nb = ~core & (best < np.iinfo(np.int64).max)
    lab[nb] = best[nb]
    roots = np.unique(lab[lab >= 0])
    out = np.full(n, -1, dtype=np.int64)
    out[lab >= 0] = np.searchsorted(roots, lab[lab >= 0])
    return out


def test_dbscan_at_size_against_grid_oracle():
    from frisk_amd.projection import dbscan
    rs = np.random.RandomState(5)
    centres = [(0, 0), (6, 0), (12, 3), (3, 9), (9, 9)]
    Y = np.vstack([rs.normal(c, 1.0, size=(36000, 2)) for c in centres] + [rs.uniform(-4, 16, size=(20000, 2))])
    Y = Y[rs.permutation(len(Y))]
    eps = 0.06
    got = dbscan(Y, eps, 50)
    want = _dbscan_oracle(Y, eps, 50)
    assert len(set(want.tolist())) > 3 and (want == -1).any() and (want >= 0).sum() > 50000
    assert np.array_equal(got, want)
    assert np.array_equal(dbscan(Y, eps, 50), got)


# ------------------------------------------------------------------------------------------------ k-means
def _same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("case", sorted(G["kmeans"]))
def test_kmeans_matches_sklearn_golden(case):
    from frisk_amd.projection import kmeans
    g = G["kmeans"][case]
    Y = A(g["Y"])
    r = kmeans(Y, g["k"], seed=0)
    assert _same_partition(r.labels, A(g["labels"]))
    assert abs(r.inertia - g["inertia"]) <= 1e-9 * g["inertia"]
    r2 = kmeans(Y, g["k"], seed=0)
    assert r2.labels.tobytes() == r.labels.tobytes() and r2.centers.tobytes() == r.centers.tobytes() and r2.inertia == r.inertia
    first = [int(x) for x in dict.fromkeys(r.labels.tolist())]
    assert first == list(range(g["k"]))                       # numbered by first occurrence in row order


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_rejects_bad_input():
    from frisk_amd import _ffi
    L = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    X = np.random.RandomState(0).uniform(size=(20, 5))
    bad = X.copy()
    bad[3, 2] = np.nan
    inf = X.copy()
    inf[0, 0] = np.inf
    mean, cov, Y = np.zeros(5), np.zeros((5, 5)), np.zeros((20, 6))
    V = np.zeros((5, 6))
    lab, cen = np.zeros(20, np.int32), np.zeros((21, 5))
    ine, it = C.c_double(), C.c_int32()
    E = _ffi.E_ARG
    assert L.frisk_proj_cov(0, p(X), 0, 5, p(mean), p(cov)) == E                               # n < 1
    assert L.frisk_proj_cov(0, p(bad), 20, 5, p(mean), p(cov)) == E                            # NaN in X
    assert L.frisk_proj_cov(0, p(inf), 20, 5, p(mean), p(cov)) == E                            # inf in X
    assert L.frisk_proj_transform(0, p(X), p(mean), p(V), 20, 5, 6, p(Y)) == E                 # d > f
    assert L.frisk_proj_transform(0, p(X), p(mean), p(V), 0, 5, 2, p(Y)) == E                  # n < 1
    assert L.frisk_proj_transform(0, p(bad), p(mean), p(V), 20, 5, 2, p(Y)) == E
    for eps in (0.0, -1.0, float("nan")):
        assert L.frisk_dbscan(0, p(X), 20, 5, eps, 5, p(lab)) == E                             # eps <= 0 or NaN
    assert L.frisk_dbscan(0, p(X), 0, 5, 1.0, 5, p(lab)) == E
    assert L.frisk_dbscan(0, p(bad), 20, 5, 1.0, 5, p(lab)) == E
    for k in (0, 21):                                                                           # k < 1, k > n
        assert L.frisk_kmeans(0, p(X), 20, 5, k, p(cen), 10, 1e-4, p(lab), p(cen), C.byref(ine), C.byref(it)) == E
    assert L.frisk_kmeans(0, p(X), 0, 5, 2, p(X), 10, 1e-4, p(lab), p(cen), C.byref(ine), C.byref(it)) == E
    assert L.frisk_kmeans(0, p(bad), 20, 5, 2, p(X), 10, 1e-4, p(lab), p(cen), C.byref(ine), C.byref(it)) == E
    # and the same calls with good input succeed
    assert L.frisk_proj_cov(0, p(X), 20, 5, p(mean), p(cov)) == _ffi.OK
    assert L.frisk_kmeans(0, p(X), 20, 5, 2, p(X), 10, 1e-4, p(lab), p(cen), C.byref(ine), C.byref(it)) == _ffi.OK


# ------------------------------------------------------------------------------------------------ CLI
def _run_cli(args, tmp):
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, G["e2e"]["fasta"]), "-t", str(tmp)] + args
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_pca_dbscan_writes_cluster_gff(tmp_path):
    """python -m frisk_amd --runProjection PCA --cluster DBSCAN --gffOutfile a.gff3 on the fixture: the reference's
    cluster-labelled GFF3 byte for byte, and a.gff3 of the unmerged anomalous windows (L1672-1675)."""
    e = G["e2e"]
    out = tmp_path / "T"
    _run_cli(e["argv"], out)
    assert sorted(os.listdir(out)).count(e["cluster_gff_name"]) == 1
    assert open(out / e["cluster_gff_name"]).read() == e["cluster_gff"]
    got = open(out / "a.gff3").read().splitlines()
    want = e["anomaly_gff"].splitlines()
    assert len(got) == len(want) == e["n_anomalous"] + 1 and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        gf, wf = g.split("\t"), w.split("\t")
        assert gf[:8] == wf[:8]
        gid, gk = gf[8].split(";")
        wid, wk = wf[8].split(";")
        # the window's KLD as the score table prints it (12 significant digits); the reference's value to 1e-11
        assert gid == wid and gk.startswith("KLD=") and abs(float(gk[4:]) - float(wk[4:])) <= 1e-11


def test_cli_unavailable_clustering_writes_no_cluster_gff(tmp_path):
    e = G["e2e"]
    out = tmp_path / "T"
    argv = list(e["argv"])
    argv[argv.index("DBSCAN")] = "SPECTRAL"
    p = _run_cli(argv, out)
    assert "--cluster is not available in this build" in p.stderr
    assert [f for f in os.listdir(out) if "cluster_labeled" in f] == []
    assert os.path.isfile(out / "a.gff3")
