"""No-GPU checks of the projection / clustering step (reference L1556-1697): the cluster-labelled GFF3 writer against the
reference's own cluster2df + anomClust2gff text, k-means++ seeding against a numpy restatement of sklearn's, the cluster GFF3's
file name, and the methods that stay unavailable."""
import json
import os

import numpy as np
import pytest

from golden_util import GOLD

G = json.load(open(os.path.join(GOLD, "projection_cluster.json")))


def A(name):
    """an array of the golden (tests/golden/projection_cluster/<name>)"""
    return np.load(os.path.join(GOLD, "projection_cluster", name))


@pytest.mark.parametrize("case", sorted(G["writers"]))
def test_cluster_gff_writer_matches_reference_text(case):
    from frisk_amd import postprocess as pp
    w = G["writers"][case]
    labels = np.array([[x] for x in w["labels"]])
    assert "".join(pp.anomClust2gff(pp.cluster_rows(labels, w["y_pred"]))) == w["gff"]


def test_cluster_gff_writer_end_to_end_labels():
    """The fixture's labels and sklearn's DBSCAN labels give the reference's cluster GFF3, byte for byte (noise present, so the
    first real cluster is Class_1)."""
    from frisk_amd import postprocess as pp
    e = G["e2e"]
    y_pred = A(e["y_pred"])
    assert -1 in y_pred and e["cluster_gff"].count("\tClass_1\t") > 0 and "\tClass_0\t" not in e["cluster_gff"]
    labels = A(e["labels"])[:, None]
    assert "".join(pp.anomClust2gff(pp.cluster_rows(labels, y_pred))) == e["cluster_gff"]


def _sklearn_plusplus(X, k, rs):
    """sklearn.cluster._kmeans._kmeans_plusplus with unit weights, restated: the chosen indices."""
    n = X.shape[0]
    trials = 2 + int(np.log(k))
    w = np.ones(n)
    first = rs.choice(n, p=w / w.sum())
    ids = [first]
    d2 = ((X - X[first]) ** 2).sum(1)
    pot = d2 @ w
    for _ in range(1, k):
        r = rs.uniform(size=trials) * pot
        cand = np.clip(np.searchsorted(np.cumsum(w * d2), r), None, n - 1)
        dc = np.minimum(d2, ((X[cand][:, None, :] - X[None, :, :]) ** 2).sum(2))
        pots = dc @ w
        b = int(np.argmin(pots))
        pot, d2 = pots[b], dc[b]
        ids.append(cand[b])
    return np.array(ids)


@pytest.mark.parametrize("k", [1, 2, 3, 7])
def test_kmeans_plusplus_seeding_matches_restatement(k):
    from frisk_amd.projection import kmeans_plusplus
    X = np.random.RandomState(3).normal(size=(400, 3)) * np.array([1.0, 4.0, 0.5])
    for seed in range(4):
        rs_a, rs_b = np.random.RandomState(seed), np.random.RandomState(seed)
        for _ in range(3):                       # n_init starts draw from one RandomState in turn
            centres, idx = kmeans_plusplus(X, k, rs_a)
            assert idx.tolist() == _sklearn_plusplus(X, k, rs_b).tolist()
            assert np.array_equal(centres, X[idx])


def test_cluster_gff_file_name():
    from frisk_amd import postprocess as pp
    from frisk_amd.cli import build_parser
    base = ["-H", "x.fa", "--runProjection", "PCA", "--gffOutfile", "a.gff3"]
    a = build_parser().parse_args(base + ["--cluster", "DBSCAN"])
    assert pp.clusterGffName(a) == "PCA_DBSCAN_k_2_cluster_labeled_windows_a.gff3" == G["e2e"]["cluster_gff_name"]
    a = build_parser().parse_args(base + ["--cluster", "KMEANS", "--kClusters", "5", "--dimReduce", "features"])
    assert pp.clusterGffName(a) == "PCA_KMEANS_k_5_cluster_labeled_features_a.gff3"
    a = build_parser().parse_args(base + ["--cluster", "DBSCAN", "--kClusters", "0"])
    assert pp.clusterGffName(a) == "PCA_DBSCAN_cluster_labeled_windows_a.gff3"


@pytest.mark.parametrize("proj,clust,warned", [("PCA", "DBSCAN", False), ("PCA", "KMEANS", False), ("PCA", "SPECTRAL", True),
                                               ("NMF", "DBSCAN", True), ("SKL-TSNE", "KMEANS", True), ("MDS", None, False),
                                               (None, "DBSCAN", True)])
def test_unavailable_methods_still_warn(proj, clust, warned):
    from frisk_amd.cli import build_parser, unavailable
    argv = ["-H", "x.fa"] + (["--runProjection", proj] if proj else []) + (["--cluster", clust] if clust else [])
    got = unavailable(build_parser().parse_args(argv))
    assert (("cluster", "sklearn clustering is out of scope") in got) == warned
    assert unavailable(build_parser().parse_args(argv + ["--graphics", "g.pdf"]))[-1][0] == "graphics"


def test_projection_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    assert {"frisk_proj_cov", "frisk_proj_transform", "frisk_dbscan", "frisk_kmeans"} <= names


# ------------------------------------------------------------------------------------------------ the GPU tests' oracles
@pytest.mark.parametrize("case", sorted(G["kmeans_init"]))
def test_lloyd_restatement_matches_sklearn_golden(case):
    """proj_oracles.lloyd, the restatement the GPU k-means tests compare with (sklearn's empty-cluster relocation included),
    gives sklearn's labels, centres, inertia and n_iter_ on every explicit-init golden."""
    import proj_oracles as PO
    g = G["kmeans_init"][case]
    lab, cen, inertia, it = PO.lloyd(A(g["Y"]), A(g["init"]), g["max_iter"], g["tol"])
    want = A(g["centers"])
    assert lab.tolist() == A(g["labels"]).tolist() and it == g["n_iter"]
    assert np.abs(cen - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert abs(inertia - g["inertia"]) <= 1e-12 * max(g["inertia"], 1.0)


def test_relocation_goldens_tell_the_rules_apart():
    """The relocation goldens end elsewhere under the old rule (an empty cluster keeps its centre)."""
    import proj_oracles as PO
    for case in ("empty_one_0", "empty_one_1", "empty_two", "dups_after", "dups_before"):
        g = G["kmeans_init"][case]
        Y, C = A(g["Y"]), A(g["init"]).copy()
        trace = []
        PO.lloyd(Y, C, g["max_iter"], g["tol"], trace)
        assert any(t["empty"] for t in trace)
        old = np.full(len(Y), -1)
        for _ in range(g["max_iter"]):
            lab = np.argmin(PO.sq_dist(Y, C), axis=1)
            Cn = np.array([Y[lab == c].mean(axis=0) if (lab == c).any() else C[c] for c in range(len(C))])
            shift, C = float(np.sum((Cn - C) ** 2)), Cn
            if np.array_equal(lab, old) or shift <= g["tol"]:
                break
            old = lab
        lab = np.argmin(PO.sq_dist(Y, C), axis=1)
        assert lab.tolist() != A(g["labels"]).tolist() or not np.allclose(C, A(g["centers"])), case


@pytest.mark.parametrize("group", ["dbscan", "dbscan_edges"])
def test_bruteforce_dbscan_oracle_matches_sklearn_goldens(group):
    import proj_oracles as PO
    for case, g in sorted(G[group].items()):
        labels, _gap = PO.dbscan_oracle(A(g["Y"]), g["eps"], g.get("min_samples", G["min_samples"]))
        assert labels.tolist() == A(g["labels"]).tolist(), case


def test_covariance_tolerance_rejects_near_misses():
    """The per-entry bound of proj_oracles.cov_oracle at n = 3 000, F = 2 772 is tight enough to fail an oracle computed with
    one row dropped, and a 16 x 16 block shifted by one column, in the small-variance order-6 block as well as overall."""
    import proj_oracles as PO
    n = 3000
    X = PO.kmer_like(n, 5)
    assert X.shape[1] == 2772
    order6 = 2772 - 2080
    cols = PO.tile_edge_columns(2772)
    _, want, tol = PO.cov_oracle(X, cols)
    want = np.asarray(want, dtype=np.float64)
    _, drop, _ = PO.cov_oracle(np.delete(X, 1234, axis=0), cols)
    bad = np.abs(np.asarray(drop, dtype=np.float64) - want) > tol
    small = np.ix_(cols >= order6, cols >= order6)
    assert bad.mean() > 0.5 and bad[small].mean() > 0.5
    # a 16 x 16 block of order-6 features (rows 2000..2015, columns 2736..2751) against the same block one column over
    blk = np.r_[2000:2016, 2736:2753]
    _, c, t = PO.cov_oracle(X, blk)
    c = np.asarray(c, dtype=np.float64)
    right, shifted, bound = c[:16, 16:32], c[:16, 17:33], t[:16, 16:32]
    assert (np.abs(shifted - right) > bound).mean() > 0.9
    # and the bound is not vacuous: the float64 two-pass product stays inside it
    Xc = X[:, cols] - X.mean(axis=0)[cols]
    assert np.all(np.abs((Xc.T @ Xc) / (n - 1) - want) <= tol)
