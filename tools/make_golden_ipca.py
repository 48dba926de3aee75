#!/usr/bin/env python3
"""Goldens of the IncrementalPCA projection (sklearn.decomposition.IncrementalPCA(n_components=d, whiten=False, copy=True,
batch_size=None).fit(X).transform(X), called at frisk/__init__.py L1629-1631): tests/golden/ipca.json and one compressed .npz per
case under tests/golden/ipca/.

No large X is stored: every random input is regenerated from the RandomState call recorded in the case (make_X of
make_golden_mds.py: Dirichlet blobs shaped like k-mer proportions) and its sha256 is recorded.  Per case:
  * the batch sizes (gen_batches(n, batch_size or 5 F, min_batch_size=d));
  * after every batch of chained partial_fit calls (asserted equal to fit): mean_, var_, components_, singular_values_,
    explained_variance_, explained_variance_ratio_, noise_variance_;
  * the final Y = transform(X);
  * gap: the smallest (lambda_i - lambda_(i+1)) / lambda_1, i <= d, of the stacked matrix of any batch (a case is kept only if
    it is >= 1e-4: the eigenvectors are then well conditioned);
  * sign_margin per batch and component: (largest - second largest) / largest of |entries| (below 1e-6 the sign rule is decided
    by rounding, and the tests compare that component up to sign);
  * pca_distance: max|Y - Y_PCA| / max|Y| up to the sign of each column (a multi-batch case is kept only if it is >= 1e-6, so
    that an alias of PCA fails the tests).
Plus the CLI end to end on tests/golden/inputs/proj_islands.fa with --runProjection IncrementalPCA at --pcaMax 3 (one batch) and
--pcaMax 2 (four batches).  This script does not use the package under test.

    python tools/make_golden_ipca.py
"""
import hashlib
import json
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_mds as MGM  # noqa: E402
import make_golden_projection as MGP  # noqa: E402

GOLD, INP = MG.GOLD, MG.INP
ARR = os.path.join(GOLD, "ipca")
MIN_SAMPLES = MGP.MIN_SAMPLES
MIN_GAP, MIN_PCA_DISTANCE, MARGIN = 1e-4, 1e-6, 1e-6
O12, O44, O2772 = (2, 10), MGM.ORDERS_44, MGM.ORDERS_2772

# name: (n, orders, spread, d, batch_size, seed)
CASES = {
    "one44": (150, O44, 60.0, 2, None, 1),
    "multi44": (1000, O44, 60.0, 2, None, 2),
    "multi44_d3": (700, O44, 60.0, 3, None, 3),
    "f2772_one": (150, O2772, 200.0, 2, None, 4),
    "f2772_b64": (400, O2772, 200.0, 2, 64, 5),
    "f12": (198, O12, 60.0, 2, None, 6),
    "d1": (500, O44, 60.0, 1, 100, 7),
    "d8": (600, O44, 60.0, 8, 50, 8),
    "tail": (223, O44, 60.0, 2, 220, 9),
    "merged_tail": (221, O44, 60.0, 2, 220, 10),
    # padding edges: F and the rows of the stacked matrix (b first, then d + b + 1) one below, at and one above multiples of the
    # Gram kernel's tile (64 columns) and K step (16 rows)
    "edge_f63_b15": (46, (2, 10, 51), 60.0, 2, 15, 11),
    "edge_f64_b16": (49, (2, 10, 52), 60.0, 2, 16, 12),
    "edge_f65_b17": (52, (2, 10, 53), 60.0, 2, 17, 13),
    "edge_f127_b12": (37, (2, 10, 115), 60.0, 2, 12, 14),
    "edge_f128_b13": (40, (2, 10, 116), 60.0, 2, 13, 15),
    "edge_b61": (184, O44, 60.0, 2, 61, 16),
    "edge_b63": (190, O44, 60.0, 2, 63, 17),
    "edge_b64": (193, O44, 60.0, 2, 64, 18),
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def sign_margin(comps):
    a = np.sort(np.abs(comps), axis=1)
    return (a[:, -1] - a[:, -2]) / a[:, -1] if comps.shape[1] > 1 else np.ones(comps.shape[0])


def run_case(X, d, batch_size, arrays, prefix=""):
    """Chained partial_fit, asserted equal to fit; the states after every batch into arrays.  Returns the json part."""
    from sklearn.decomposition import PCA, IncrementalPCA
    from sklearn.utils import gen_batches
    n, f = X.shape
    size = 5 * f if batch_size is None else batch_size
    batches = [(s.start, s.stop) for s in gen_batches(n, size, min_batch_size=d)]
    full = IncrementalPCA(n_components=d, whiten=False, copy=True, batch_size=batch_size).fit(X)
    ip = IncrementalPCA(n_components=d, whiten=False, copy=True, batch_size=batch_size)
    gap, noise, margins = np.inf, [], []
    for k, (lo, hi) in enumerate(batches):
        Xb = X[lo:hi]
        # the spectrum of the stacked matrix of this batch, rebuilt from sklearn's state before it
        if k == 0:
            A = Xb - Xb.mean(axis=0)
        else:
            T = Xb.mean(axis=0)
            corr = np.sqrt((ip.n_samples_seen_ / (ip.n_samples_seen_ + hi - lo)) * (hi - lo)) * (ip.mean_ - T)
            A = np.vstack((ip.singular_values_.reshape(-1, 1) * ip.components_, Xb - T, corr))
        lam = np.linalg.svd(A, compute_uv=False) ** 2
        lam = np.concatenate([lam, np.zeros(max(0, d + 1 - len(lam)))]) if f > d else lam
        top = lam[:d + 1] if len(lam) > d else lam
        if len(top) > 1:
            gap = min(gap, float(np.min(top[:-1] - top[1:]) / lam[0]))
        ip.partial_fit(Xb.copy())
        assert np.allclose(ip.singular_values_ ** 2, lam[:d], rtol=1e-9)
        for key, val in (("mean", ip.mean_), ("var", ip.var_), ("comps", ip.components_), ("S", ip.singular_values_),
                         ("ev", ip.explained_variance_), ("evr", ip.explained_variance_ratio_)):
            arrays[prefix + "%s_%d" % (key, k)] = np.array(val)
        noise.append(float(ip.noise_variance_))
        margins.append(sign_margin(ip.components_))
    assert ip.n_samples_seen_ == full.n_samples_seen_ == n
    for key in ("mean_", "var_", "components_", "singular_values_", "explained_variance_", "explained_variance_ratio_"):
        assert np.array_equal(getattr(ip, key), getattr(full, key)), key
    assert ip.noise_variance_ == full.noise_variance_
    Y = full.transform(X)
    Yp = PCA(n_components=d, svd_solver="full").fit(X).transform(X)
    dist = max(min(np.max(np.abs(Y[:, q] - Yp[:, q])), np.max(np.abs(Y[:, q] + Yp[:, q]))) for q in range(d)) / np.max(np.abs(Y))
    arrays[prefix + "Y"] = Y
    arrays[prefix + "noise"] = np.array(noise)
    arrays[prefix + "sign_margin"] = np.array(margins)
    return {"batch_sizes": [hi - lo for lo, hi in batches], "gap": gap, "pca_distance": float(dist),
            "min_sign_margin": float(np.min(margins))}


def make_case(name, n, orders, spread, d, batch_size, seed):
    X = MGM.make_X(n, orders, spread, 0, seed)
    arrays = {}
    g = run_case(X, d, batch_size, arrays)
    g.update({"n": n, "F": int(X.shape[1]), "d": d, "batch_size": batch_size, "file": name + ".npz",
              "X": {"n": n, "orders": list(orders), "spread": spread, "seed": seed, "sha256": sha(X)}})
    assert g["gap"] >= MIN_GAP, (name, g["gap"])
    assert len(g["batch_sizes"]) == 1 or g["pca_distance"] >= MIN_PCA_DISTANCE, (name, g["pca_distance"])
    np.savez_compressed(os.path.join(ARR, g["file"]), **arrays)
    return g


def batch_rule_cases():
    """Recorded sklearn.utils.gen_batches outputs: (n, batch_size, min_batch_size) -> batch sizes."""
    from sklearn.utils import gen_batches
    out = []
    for n, size, mn in ((1000, 220, 2), (223, 220, 2), (221, 220, 2), (222, 220, 2), (220, 220, 2), (440, 220, 2), (441, 220, 2),
                        (150, 220, 2), (1, 220, 1), (7, 3, 1), (7, 3, 2), (8, 3, 3), (9, 3, 8), (600, 50, 8), (30000, 13860, 2),
                        (100000, 13860, 2), (198, 60, 2), (5, 10, 0)):
        out.append({"n": n, "batch_size": size, "min_batch_size": mn,
                    "sizes": [s.stop - s.start for s in gen_batches(n, size, min_batch_size=mn)]})
    return out


def end_to_end(ns, pmax, tag):
    """The fixture through IncrementalPCA(n_components=2) and DBSCAN at an eps in the middle of the range that gives three clusters
    and noise, no pair distance within 1e-6 eps of it."""
    from sklearn.cluster import DBSCAN
    (m, k, w, inc, pmin, pmax, force, args, anomWin, n_windows), anomLabels, anomCounts = MGM.anomalies(ns, pmax)
    dims = 2
    arrays = {}
    g = run_case(anomCounts, dims, None, arrays)
    Y = arrays["Y"]
    pair = np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(Y), 1)]
    grid = np.geomspace(np.percentile(pair, 0.5), np.percentile(pair, 50), 400)
    good = []
    for e in grid:
        e = float("%.4g" % e)
        lab = DBSCAN(eps=e, min_samples=MIN_SAMPLES).fit(Y).labels_
        if np.min(np.abs(pair - e)) <= MARGIN * e:
            continue
        if len(set(lab.tolist()) - {-1}) == 3 and (lab == -1).any():
            good.append((e, lab))
    assert good, "no eps gives three clusters and noise"
    eps, y_pred = good[len(good) // 2]
    np.savez_compressed(os.path.join(ARR, "e2e_%s.npz" % tag), **arrays)
    argv = ["-m", str(m), "-k", str(k), "-w", str(w), "-i", str(inc), "-F", repr(force), "--runProjection", "IncrementalPCA",
            "--projectionDims", str(dims), "--pcaMin", str(pmin), "--pcaMax", str(pmax), "--cluster", "DBSCAN",
            "--epsDBSCAN", repr(eps), "--gffOutfile", "a.gff3"]
    g.update({"fasta": MGP.FASTA, "argv": argv, "forceThresholdKLD": force, "epsDBSCAN": eps, "n_windows": n_windows,
              "n_anomalous": len(anomLabels), "F": int(anomCounts.shape[1]), "n_noise": int(np.sum(y_pred == -1)),
              "clusters": len(set(y_pred.tolist()) - {-1}), "anomCounts_sha256": sha(anomCounts), "file": "e2e_%s.npz" % tag,
              "cluster_gff_name": "IncrementalPCA_DBSCAN_k_2_cluster_labeled_windows_a.gff3",
              "kmeans_gff_name": "IncrementalPCA_KMEANS_k_2_cluster_labeled_windows_a.gff3",
              "cluster_gff": "".join(ns["anomClust2gff"](ns["cluster2df"](Y, labels=anomLabels, y_pred=y_pred))),
              "anomaly_gff": "".join(ns["anomaly2GFF"](anomWin, args))})
    assert g["gap"] >= MIN_GAP and (len(g["batch_sizes"]) == 1 or g["pca_distance"] >= MIN_PCA_DISTANCE)
    return g


def main():
    import sklearn
    MGP._patch_pandas()
    if os.path.isdir(ARR):
        for f in os.listdir(ARR):
            if f.endswith(".npz"):
                os.remove(os.path.join(ARR, f))
    os.makedirs(ARR, exist_ok=True)
    cases = {}
    for name, c in CASES.items():
        g = cases[name] = make_case(name, *c)
        print("%-14s n %4d F %4d d %d: batches %s, gap %.2e, min sign margin %.1e, PCA distance %.1e, %d KB"
              % (name, g["n"], g["F"], g["d"], g["batch_sizes"], g["gap"], g["min_sign_margin"], g["pca_distance"],
                 os.path.getsize(os.path.join(ARR, g["file"])) // 1024), flush=True)
    ns = MG.load_reference_functions(extra=("getBEDSeq", "cluster2df", "anomClust2gff"))
    e2e = {}
    for tag, pmax in (("pcamax3", 3), ("pcamax2", 2)):
        e = e2e[tag] = end_to_end(ns, pmax, tag)
        print("e2e %s: %d anomalous windows, F %d, batches %s, eps %s, %d clusters, %d noise, gap %.2e, PCA distance %.1e, "
              "min sign margin %.1e" % (tag, e["n_anomalous"], e["F"], e["batch_sizes"], e["epsDBSCAN"], e["clusters"], e["n_noise"],
                                        e["gap"], e["pca_distance"], e["min_sign_margin"]))
    doc = {"sklearn": sklearn.__version__, "min_samples": MIN_SAMPLES, "min_gap": MIN_GAP, "min_pca_distance": MIN_PCA_DISTANCE,
           "cases": cases, "gen_batches": batch_rule_cases(), "e2e": e2e}
    with open(os.path.join(GOLD, "ipca.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
