#!/usr/bin/env python3
"""Goldens of the MDS projection (sklearn.manifold.MDS(metric=True, n_init=5, max_iter=500, eps=0.001, n_jobs=1,
dissimilarity='euclidean'), called at frisk/__init__.py L1624-1627): tests/golden/mds.json and one compressed .npz per case under
tests/golden/mds/.

No large X is stored: every random input is regenerated from the RandomState call recorded in the case (see make_X) and its
sha256 is recorded, so the tests rebuild it the same way and check the hash.  Per case:
  * sklearn's euclidean_distances(X) (the Gram form) on a sample of rows, the direct-difference D on the same rows and the sum
    of the whole direct-difference D (D_sum);
  * the n_init starts, drawn in turn from RandomState(seed) as smacof(n_jobs=1) draws them;
  * every start's states Y_t and raw stresses from chained _smacof_single(D_direct, init=Y_t, max_iter=1) calls, asserted equal
    to sklearn's own run of that start;
  * smacof(D_direct, n_init, max_iter, eps, random_state=seed, n_jobs=1): what the GPU computes, on the same D;
  * MDS(..., random_state=seed).fit_transform(X): end to end, with sklearn's Gram-form D;
  * the decision margins: |ratio - eps| / eps of every stop check of every start and the relative stress gap between the
    best start and the runner-up.  A case is kept only if both are >= 1e-6.
Plus the CLI end to end on tests/golden/inputs/proj_islands.fa with --runProjection MDS.  This script does not use the package
under test.

    python tools/make_golden_mds.py
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
import make_golden_projection as MGP  # noqa: E402

GOLD, INP = MG.GOLD, MG.INP
ARR = os.path.join(GOLD, "mds")
MIN_SAMPLES = MGP.MIN_SAMPLES
MARGIN = 1e-6
N_INIT, MAX_ITER, EPS = 5, 500, 1e-3
ORDERS_44 = (2, 10, 32)                                 # kept words of orders 1..3 (--pcaMin 1 --pcaMax 3): F = 44
ORDERS_2772 = (2, 10, 32, 136, 512, 2080)               # orders 1..6: F = 2 772
SAMPLE_ROWS = 8

# name: (n, orders, spread, dims, dups, max_iter, eps, seed)
CASES = {
    "blobs44": (150, ORDERS_44, 60.0, 2, 0, MAX_ITER, EPS, 1),
    "f2772": (150, ORDERS_2772, 200.0, 2, 0, MAX_ITER, EPS, 2),
    "dups": (160, ORDERS_2772, 200.0, 2, 24, MAX_ITER, EPS, 3),
    "d1": (120, ORDERS_44, 60.0, 1, 0, MAX_ITER, EPS, 4),
    "d3": (120, ORDERS_44, 60.0, 3, 0, MAX_ITER, EPS, 5),
    "d64": (12, ORDERS_44, 60.0, 64, 0, MAX_ITER, EPS, 6),
    "n2": (2, ORDERS_44, 60.0, 2, 0, MAX_ITER, EPS, 7),
    "n3": (3, ORDERS_44, 60.0, 2, 0, MAX_ITER, EPS, 8),
    "n65": (65, ORDERS_44, 60.0, 2, 0, MAX_ITER, EPS, 9),
    "n129": (129, ORDERS_44, 60.0, 2, 0, MAX_ITER, EPS, 10),
    "maxiter": (100, ORDERS_44, 60.0, 2, 0, 30, 0.0, 11),
    "eps1e-6": (50, ORDERS_44, 60.0, 2, 0, MAX_ITER, 1e-6, 12),
}


def make_X(n, orders, spread, dups, seed):
    """Dirichlet blobs of k-mer-proportion-like rows from RandomState(seed): 3 blobs, a centre per order, rows Dirichlet around
    it in blob order, then a permutation; the last `dups` rows are replaced by copies of rows drawn from the others."""
    rs = np.random.RandomState(seed)
    sizes = [n // 3 + (1 if b < n % 3 else 0) for b in range(3)]
    rows = []
    for m in sizes:
        centre = [rs.dirichlet(np.full(w, 2.0)) for w in orders]
        for _ in range(m):
            rows.append(np.concatenate([rs.dirichlet(c * spread + 1e-3) for c in centre]))
    X = np.array(rows)[rs.permutation(n)]
    if dups:
        X[n - dups:] = X[rs.randint(0, n - dups, dups)]
    return X


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def direct_D(X):
    n = X.shape[0]
    D = np.empty((n, n))
    for i in range(n):
        D[i] = np.sqrt(((X[i] - X) ** 2).sum(axis=1))
    np.fill_diagonal(D, 0.0)
    return np.maximum(D, D.T)       # exactly symmetric (each pair's two sums agree up to the summation order of numpy)


def chain(D, Y0, max_iter, eps):
    """One start step by step: _smacof_single(init=Y_t, max_iter=1) chained, the stop rule applied here, asserted equal to the
    full _smacof_single.  Returns (states Y_0 .. Y_T, stresses of Y_1 .. Y_T, T, stop ratios of every check)."""
    from sklearn.manifold._mds import _smacof_single
    from sklearn.metrics import euclidean_distances
    Ys, st, ratios = [Y0], [], []
    old = None
    for it in range(max_iter):
        Y, s, _ = _smacof_single(D, metric=True, n_components=Y0.shape[1], init=Ys[-1], max_iter=1, eps=eps)
        Ys.append(Y)
        st.append(s)
        if old is not None:
            r = (old - s) / ((euclidean_distances(Y).ravel() ** 2).sum() / 2)
            ratios.append(r)
            if r < eps:
                break
        old = s
    T = len(st)
    Yf, sf, nf = _smacof_single(D, metric=True, n_components=Y0.shape[1], init=Y0, max_iter=max_iter, eps=eps)
    assert nf == T and sf == st[-1] and np.array_equal(Yf, Ys[-1]), (nf, T)
    return Ys, st, T, ratios


def margins(ratios, eps):
    if eps == 0.0:      # eps = 0 stops only when the stress rises: every ratio must be clearly positive
        return [abs(r) / 1e-12 for r in ratios]
    return [abs(r - eps) / eps for r in ratios]


def run_case(X, dims, max_iter, eps, seed, arrays, prefix=""):
    from sklearn.manifold import MDS, smacof
    from sklearn.metrics import euclidean_distances
    n = X.shape[0]
    D = direct_D(X)
    rs = np.random.RandomState(seed)
    starts = [rs.uniform(size=n * dims).reshape(n, dims) for _ in range(N_INIT)]
    stresses, n_iters, worst = [], [], np.inf
    for k, Y0 in enumerate(starts):
        Ys, st, T, ratios = chain(D, Y0, max_iter, eps)
        arrays[prefix + "Y0_%d" % k] = Y0
        arrays[prefix + "states_%d" % k] = np.array(Ys)
        arrays[prefix + "stress_%d" % k] = np.array(st)
        stresses.append(st[-1])
        n_iters.append(T)
        if ratios:
            worst = min(worst, min(margins(ratios, eps)))
    best = int(np.argmin(stresses))         # the first of equal minima, as smacof's strict <
    # (n = 2: every start fits D exactly and its stress is rounding noise; the tests check the fit instead of the winner)
    gap = (sorted(stresses)[1] - stresses[best]) / stresses[best] if n > 2 else np.inf
    Ysm, ssm, nsm = smacof(D, metric=True, n_components=dims, n_init=N_INIT, max_iter=max_iter, eps=eps, random_state=seed,
                           n_jobs=1, return_n_iter=True, normalized_stress=False)
    assert nsm == n_iters[best] and ssm == stresses[best] and np.array_equal(Ysm, arrays[prefix + "states_%d" % best][-1])
    model = MDS(n_components=dims, metric=True, n_init=N_INIT, max_iter=max_iter, eps=eps, n_jobs=1, random_state=seed,
                dissimilarity="euclidean", normalized_stress=False)
    Ymds = model.fit_transform(X)
    arrays[prefix + "Y_mds"] = Ymds
    Dsk = euclidean_distances(X)
    return {"best_start": best, "stresses": stresses, "n_iters": n_iters, "stress": float(ssm), "n_iter": int(nsm),
            "mds_stress": float(model.stress_), "mds_n_iter": int(model.n_iter_), "stop_margin": float(worst),
            "best_gap": float(gap), "D_sum": float(D.sum())}, D, Dsk


def make_case(name, n, orders, spread, dims, dups, max_iter, eps, seed):
    X = make_X(n, orders, spread, dups, seed)
    arrays = {}
    g, D, Dsk = run_case(X, dims, max_iter, eps, seed, arrays)
    rows = np.sort(np.random.RandomState(seed + 1000).choice(n, min(n, SAMPLE_ROWS), replace=False))
    arrays["rows"] = rows
    arrays["D_rows"] = D[rows]
    arrays["Dsk_rows"] = Dsk[rows]
    g.update({"n": n, "F": int(X.shape[1]), "dims": dims, "dups": dups, "max_iter": max_iter, "eps": eps, "seed": seed,
              "X": {"n": n, "orders": list(orders), "spread": spread, "dups": dups, "seed": seed, "sha256": sha(X)},
              "file": name + ".npz", "Y_mds_gap": float(np.max(np.abs(arrays["Y_mds"] - arrays["states_%d" % g["best_start"]][-1]))
                                                       / np.max(np.abs(arrays["Y_mds"])))})
    assert g["stop_margin"] >= MARGIN and g["best_gap"] >= MARGIN, (name, g["stop_margin"], g["best_gap"])
    assert g["mds_n_iter"] == g["n_iter"], name
    np.savez_compressed(os.path.join(ARR, g["file"]), **arrays)
    return g


def coincident_case():
    """One step from a hand-built state where points 0 and 1 coincide (dyadic coordinates: sklearn's Gram-form distance of the
    pair is exactly 0 too), with nonzero D between them: the 1e-5 rule on both sides."""
    from sklearn.manifold._mds import _smacof_single
    from sklearn.metrics import euclidean_distances
    rs = np.random.RandomState(77)
    n = 12
    X = rs.rand(n, 5)
    D = direct_D(X)
    Y = rs.randint(-8, 9, size=(n, 2)) / 8.0
    Y[1] = Y[0]
    assert euclidean_distances(Y)[0, 1] == 0.0 and D[0, 1] > 0
    Y1, s1, _ = _smacof_single(D, metric=True, n_components=2, init=Y, max_iter=1, eps=0.0)
    np.savez_compressed(os.path.join(ARR, "coincident.npz"), Y=Y, Y1=Y1, D=D)
    return {"file": "coincident.npz", "n": n, "stress1": float(s1),
            "X": {"call": "RandomState(77).rand(12, 5)", "sha256": sha(X)}}


def anomalies(ns, pmax=3):
    """The fixture's anomalous windows and their symmetric k-mer proportions (orders 1..pmax), as
    make_golden_projection.end_to_end computes them."""
    import pandas as pd
    import shutil
    import tempfile
    fa = os.path.join(INP, MGP.FASTA)
    m, k, w, inc, pmin = 1, 4, 200, 100, 1
    tmp = tempfile.mkdtemp(prefix="frisk_gold_")
    a = MG.Args(fa, m=m, k=k, w=w, i=inc, tempDir=tmp)
    blank = ns["rangeMaps"](m, k)
    gk = ns["computeKmers"](a, genomepickle=ns["makePicklePath"](a, space="genome"), window=None, genomeMode=True, kmerMap=blank,
                            getMeta=True)
    shutil.rmtree(tmp)
    rows = []
    for seq, sname, start, stop in ns["crawlGenome"](a, fa):
        wk = ns["computeKmers"](a, genomepickle=None, window=[(sname, seq)], genomeMode=False, kmerMap=blank, getMeta=True)
        kld = ns["KLD"](ns["IvomBuild"](wk, a, gk, True), ns["IvomBuild"](wk, a, gk, False), a)
        rows.append((sname, start, stop, kld, ns["calcGC"](seq)))
    allWindows = pd.DataFrame(rows, columns=["name", "start", "stop", "windowKLD", "GC"])
    lk = np.sort(np.log10(allWindows["windowKLD"].values))
    hi = lk[len(lk) // 2:]
    j = int(np.argmax(np.diff(hi)))
    force = float("%.4g" % 10 ** ((hi[j] + hi[j + 1]) / 2))
    args = MGP._Args(findSelf=False, mergeDist=0, dimReduce="windows", forceThresholdKLD=force, threshTypeKLD=None,
                     percentileKLD=99.0, pcaMin=pmin, pcaMax=pmax, minWordSize=m, maxWordSize=k, maskHost=False, hostSeq=None,
                     windowlen=w)
    thr, _ = ns["setKLDThresh"](args, np.log10(allWindows[["windowKLD"]].values))
    anomWin, _ = ns["thresholdKLD"](allWindows, thr, args, threshCol="windowKLD", merge=False)
    genome = dict(ns["iterFasta"](fa))
    names, counts = [], []
    pblank = ns["rangeMaps"](pmin, pmax)
    for name, target in ns["getBEDSeq"](genome, anomWin):
        cm = ns["computeKmers"](args, genomepickle=None, window=[(name, target)], genomeMode=False, pcaMode=True, kmerMap=pblank,
                                getMeta=False, sym=True)
        counts.append(ns["flattenKmerMap"](ns["scrubMirrors"](cm), window=w, seqLen=len(target), kmin=pmin, kmax=pmax, prop=True))
        names.append([name])
    return (m, k, w, inc, pmin, pmax, force, args, anomWin, len(rows)), np.array(names), np.vstack(counts)


def end_to_end(ns):
    """The fixture through MDS(random_state=0) (the CLI's --seed default), DBSCAN at an eps in the middle of the range that gives
    three clusters and some noise, with no pair distance of either embedding (sklearn's, and smacof on the direct D) within 1e-6
    of it, and both embeddings giving the same labels."""
    from sklearn.cluster import DBSCAN
    (m, k, w, inc, pmin, pmax, force, args, anomWin, n_windows), anomLabels, anomCounts = anomalies(ns)
    dims = 2
    arrays = {}
    g, _, _ = run_case(anomCounts, dims, MAX_ITER, EPS, 0, arrays, prefix="e2e_")
    assert g["stop_margin"] >= MARGIN and g["best_gap"] >= MARGIN, (g["stop_margin"], g["best_gap"])
    Ys = [arrays["e2e_Y_mds"], arrays["e2e_states_%d" % g["best_start"]][-1]]
    dists = [np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(Y), 1)] for Y in Ys]
    grid = np.geomspace(np.percentile(dists[0], 0.5), np.percentile(dists[0], 50), 400)
    good = []
    for e in grid:
        e = float("%.4g" % e)
        labs = [DBSCAN(eps=e, min_samples=MIN_SAMPLES).fit(Y).labels_ for Y in Ys]
        if not np.array_equal(labs[0], labs[1]) or any(np.min(np.abs(dk - e)) <= MARGIN * e for dk in dists):
            continue
        if len(set(labs[0].tolist()) - {-1}) >= 2 and (labs[0] == -1).any():
            good.append((e, labs[0]))
    assert good, "no eps gives two or more clusters and noise"
    eps, y_pred = good[len(good) // 2]
    Y = Ys[0]
    cluster_gff = "".join(ns["anomClust2gff"](ns["cluster2df"](Y, labels=anomLabels, y_pred=y_pred)))
    anomaly_gff = "".join(ns["anomaly2GFF"](anomWin, args))
    argv = ["-m", str(m), "-k", str(k), "-w", str(w), "-i", str(inc), "-F", repr(force), "--runProjection", "MDS",
            "--projectionDims", str(dims), "--pcaMin", str(pmin), "--pcaMax", str(pmax), "--cluster", "DBSCAN",
            "--epsDBSCAN", repr(eps), "--gffOutfile", "a.gff3"]
    g.update({"fasta": MGP.FASTA, "argv": argv, "forceThresholdKLD": force, "epsDBSCAN": eps, "n_windows": n_windows,
              "n_anomalous": len(anomLabels), "n_noise": int(np.sum(y_pred == -1)), "clusters": len(set(y_pred.tolist()) - {-1}),
              "cluster_gff_name": "MDS_DBSCAN_k_2_cluster_labeled_windows_a.gff3",
              "kmeans_gff_name": "MDS_KMEANS_k_2_cluster_labeled_windows_a.gff3",
              "cluster_gff": cluster_gff, "anomaly_gff": anomaly_gff})
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
        print("%-8s n %4d F %4d d %2d: best start %d, n_iter %3d, n_iters %s, stop margin %.2e, best gap %.2e, Y_mds gap %.1e, "
              "%d KB" % (name, g["n"], g["F"], g["dims"], g["best_start"], g["n_iter"], g["n_iters"], g["stop_margin"],
                         g["best_gap"], g["Y_mds_gap"], os.path.getsize(os.path.join(ARR, g["file"])) // 1024), flush=True)
    ns = MG.load_reference_functions(extra=("getBEDSeq", "cluster2df", "anomClust2gff"))
    e2e = end_to_end(ns)
    print("e2e: %d anomalous windows, eps %s, %d clusters, %d noise, n_iter %d, best start %d"
          % (e2e["n_anomalous"], e2e["epsDBSCAN"], e2e["clusters"], e2e["n_noise"], e2e["n_iter"], e2e["best_start"]))
    doc = {"sklearn": sklearn.__version__, "min_samples": MIN_SAMPLES, "margin": MARGIN, "n_init": N_INIT, "cases": cases,
           "coincident": coincident_case(), "e2e": e2e}
    with open(os.path.join(GOLD, "mds.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
