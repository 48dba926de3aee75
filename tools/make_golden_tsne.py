#!/usr/bin/env python3
"""Goldens of the PY-TSNE projection (reference frisk/tsne.py, called at frisk/__init__.py L1622-1623): tests/golden/tsne.json
and one compressed .npz per case under tests/golden/tsne/.

The reference's tsne module is imported by path at generation time and run as it is; nothing of it is copied.  Its
intermediate states are read, not recomputed: a sys.settrace hook copies Y, iY and gains at the top of the chosen iterations
(and P at t = 0 and t = 101), the bisection's try count of every row and the final beta from x2p, and the PCA output that x2p
receives; a logging.Handler collects the 100 logged costs.  Y0 replaces np.random.randn for the run.  The trajectory is chaotic,
so every case also records an ensemble: the run from Y0 and from 4 copies of Y0 scaled by 1 + k 1e-13, their final costs and
the DBSCAN labels at an eps on which all five agree.  This script does not use the package under test.  Every random input is
drawn from a fixed numpy RandomState, so a rerun writes the same bytes.

    python tools/make_golden_tsne.py
"""
import hashlib
import importlib.util
import inspect
import json
import logging
import os
import re
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
import make_golden_projection as MGP  # noqa: E402

GOLD, INP = MG.GOLD, MG.INP
ARR = os.path.join(GOLD, "tsne")
TSNE_SRC = os.path.join(os.path.dirname(MG.REF_SRC), "tsne.py")
SNAP_T = (0, 1, 19, 20, 21, 99, 100, 101, 102, 500, 998, 999)      # snapshot t and t + 1 are both stored
PERTURB = 1e-13
MIN_SAMPLES = MGP.MIN_SAMPLES
ORDERS_44 = (2, 10, 32)                                 # kept words of orders 1..3 (--pcaMin 1 --pcaMax 3): F = 44
ORDERS_2772 = (2, 10, 32, 136, 512, 2080)               # orders 1..6: F = 2 772


def load_tsne():
    spec = importlib.util.spec_from_file_location("reference_tsne", TSNE_SRC)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _line_of(fn, pattern):
    src, first = inspect.getsourcelines(fn)
    hits = [first + k for k, s in enumerate(src) if re.search(pattern, s)]
    assert len(hits) == 1, (fn.__name__, pattern, hits)
    return hits[0]


class _Costs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.values = []

    def emit(self, record):
        m = re.match(r"Iteration (\d+) : error is (.*)$", record.getMessage())
        if m:
            self.values.append((int(m.group(1)), float(m.group(2))))


def run_reference(T, X, Y0, dims, perplexity, trace=True):
    """tsne.tsne(X, dims, 50, perplexity) from Y0: (final Y, costs, record of the traced states)."""
    rec = {"snap": {}, "P": {}, "tries": [], "beta": None, "Xp": None}
    want = set(SNAP_T) | {t + 1 for t in SNAP_T}
    loop_line = _line_of(T.tsne, r"sum_Y\s*=\s*np\.sum\(np\.square\(Y\)")
    row_line = _line_of(T.x2p, r"=\s*thisP;")

    def in_tsne(frame, event, arg):
        if event == "line" and frame.f_lineno == loop_line:
            t = frame.f_locals["iter"]
            if t in want:
                rec["snap"][t] = tuple(frame.f_locals[k].copy() for k in ("Y", "iY", "gains"))
            if t in (0, 101):
                rec["P"][t] = frame.f_locals["P"].copy()
        elif event == "return":
            rec["snap"][1000] = tuple(frame.f_locals[k].copy() for k in ("Y", "iY", "gains"))
        return in_tsne

    def in_x2p(frame, event, arg):
        if event == "call":
            rec["Xp"] = frame.f_locals["X"].copy()
        elif event == "line" and frame.f_lineno == row_line:
            rec["tries"].append(int(frame.f_locals["tries"]))
        elif event == "return":
            rec["beta"] = frame.f_locals["beta"][:, 0].copy()
        return in_x2p

    def tracer(frame, event, arg):
        if frame.f_code is T.tsne.__code__:
            return in_tsne
        if frame.f_code is T.x2p.__code__:
            return in_x2p(frame, event, arg)
        return None

    costs = _Costs()
    root = logging.getLogger()
    root.addHandler(costs)
    saved = np.random.randn
    np.random.randn = lambda *shape: Y0.copy()
    try:
        if trace:
            sys.settrace(tracer)
        Y = T.tsne(X=X, no_dims=dims, initial_dims=50, perplexity=perplexity)
    finally:
        sys.settrace(None)
        np.random.randn = saved
        root.removeHandler(costs)
    assert [t for t, _ in costs.values] == list(range(10, 1001, 10))
    return Y, np.array([c for _, c in costs.values]), rec


def _memo_pca(T):
    """tsne() calls pca() once per run; the ensemble members share one input, so its (deterministic) result is kept."""
    orig, memo = T.pca, {}

    def pca(X=np.array([]), no_dims=50):
        key = (X.tobytes(), no_dims)
        if key not in memo:
            memo[key] = orig(X, no_dims)
        return memo[key].copy()
    T.pca = pca


def eig_order_ok(X, keep=50):
    """The reference's pca keeps eig's first `keep` columns: a case is usable only when they are the top-`keep` eigenvalues
    as a set and the gap after them is clear (then any eigensolver keeps the same subspace)."""
    Xc = X - np.tile(np.mean(X, 0), (X.shape[0], 1))
    lam = np.linalg.eig(np.dot(Xc.T, Xc))[0].real
    order = np.argsort(-lam, kind="stable")
    gap = (lam[order[keep - 1]] - lam[order[keep]]) / lam[order[0]]
    return set(order[:keep].tolist()) == set(range(keep)), float(gap)


def blobs(rs, sizes, orders, spread):
    """Rows of k-mer-proportion-like data: per blob a Dirichlet centre per order, rows Dirichlet around it."""
    rows = []
    for m in sizes:
        centre = [rs.dirichlet(np.full(w, 2.0)) for w in orders]
        for _ in range(m):
            rows.append(np.concatenate([rs.dirichlet(c * spread + 1e-3) for c in centre]))
    X = np.array(rows)
    return X[rs.permutation(len(X))]


def _same_partition(a, b):
    if not np.array_equal(a == -1, b == -1):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})


def choose_eps(Ys, n_blobs):
    """An eps on which the DBSCAN labels of every ensemble member agree (up to renaming), no pair distance of any member within
    1e-6 of it (relative): the middle of the longest run of such eps on a grid, preferring runs with n_blobs clusters."""
    from sklearn.cluster import DBSCAN
    dists = [np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(Y), 1)] for Y in Ys]
    grid = np.geomspace(np.percentile(dists[0], 0.5), np.percentile(dists[0], 60), 300)
    ok = []
    for e in grid:
        e = float("%.4g" % e)
        labs = [DBSCAN(eps=e, min_samples=MIN_SAMPLES).fit(Y).labels_ for Y in Ys]
        agree = all(_same_partition(labs[0], l) for l in labs[1:]) and all(np.min(np.abs(d - e)) > 1e-6 * e for d in dists)
        ok.append((e, agree, len(set(labs[0].tolist()) - {-1})))
    runs, cur = [], []
    for e, agree, k in ok:
        if agree and (not cur or cur[-1][1] == k):
            cur.append((e, k))
        else:
            if cur:
                runs.append(cur)
            cur = [(e, k)] if agree else []
    if cur:
        runs.append(cur)
    assert runs, "no eps on which the ensemble agrees"
    runs.sort(key=lambda r: (r[0][1] != n_blobs, -len(r)))
    best = runs[0]
    return best[len(best) // 2][0]


CASES = [
    # name, sizes of the blobs, feature orders, spread, dims, perplexity, duplicated rows
    ("blobs3", (70, 70, 70), ORDERS_44, 300.0, 2, 20.0, 0),
    ("blobs4_p5", (60, 60, 60, 60), ORDERS_44, 300.0, 2, 5.0, 0),
    ("blobs3_p50", (70, 70, 70), ORDERS_44, 300.0, 2, 50.0, 0),
    ("d1", (60, 60, 60), ORDERS_44, 300.0, 1, 20.0, 0),
    ("d3", (60, 60, 60), ORDERS_44, 300.0, 3, 20.0, 0),
    ("dups", (60, 60), ORDERS_44, 300.0, 2, 20.0, 30),
    ("f2772", (67, 67, 66), ORDERS_2772, 3000.0, 2, 20.0, 0),
    ("n5", (5,), ORDERS_44, 300.0, 2, 20.0, 0),
]


def make_case(T, seed, name, sizes, orders, spread, dims, perplexity, dups):
    from sklearn.cluster import DBSCAN
    rs = np.random.RandomState(seed)
    X = blobs(rs, sizes, orders, spread)
    if dups:
        src = rs.choice(len(X), dups, replace=False)
        dst = rs.choice(np.setdiff1d(np.arange(len(X)), src), dups, replace=False)
        X[dst] = X[src]
    n, F = X.shape
    doc = {"n": n, "F": F, "dims": dims, "perplexity": perplexity, "blobs": len(sizes), "seed": seed}
    if F > 50:
        same, gap = eig_order_ok(X)
        assert same and gap > 1e-6, (name, same, gap)
        doc["eig_gap_at_50"] = gap
    Y0 = np.random.RandomState(seed + 1).randn(n, dims)
    Y, cost, rec = run_reference(T, X, Y0, dims, perplexity)
    assert np.array_equal(rec["snap"][1000][0], Y)
    arrays = {"Xp": rec["Xp"], "Y0": Y0, "beta": rec["beta"], "tries": np.array(rec["tries"], dtype=np.int32),
              "cost": cost, "Y_final": Y}
    if F <= 50:
        arrays["X"] = X
    else:                                               # 4.4 MB: regenerated from the seed by blobs(), checked by its digest
        doc["X_sha256"] = hashlib.sha256(X.tobytes()).hexdigest()
    if n <= 300:
        arrays["q"] = rec["P"][101]                     # the reference's P after "P = P / 4": q
    if name == "blobs3":
        arrays["P0"] = rec["P"][0]                      # the exaggerated P of iterations 0..100
    for t, (y, iy, g) in sorted(rec["snap"].items()):
        arrays["Y_%d" % t], arrays["iY_%d" % t], arrays["gains_%d" % t] = y, iy, g
    finals, costs = [Y], [cost[-1]]
    for k in range(1, 5):
        Yk, ck, _ = run_reference(T, X, Y0 * (1.0 + k * PERTURB), dims, perplexity, trace=False)
        finals.append(Yk)
        costs.append(ck[-1])
    eps = choose_eps(finals, len(sizes))
    labels = DBSCAN(eps=eps, min_samples=MIN_SAMPLES).fit(Y).labels_.astype(np.int32)
    arrays["labels"] = labels
    doc.update({"snapshots": list(SNAP_T), "eps": eps, "ensemble_final_cost": [float(c) for c in costs],
                "clusters": len(set(labels.tolist()) - {-1}), "noise": int(np.sum(labels == -1)),
                "tries_max": int(np.max(rec["tries"])), "file": name + ".npz"})
    np.savez_compressed(os.path.join(ARR, name + ".npz"), **arrays)
    return doc


def end_to_end(T, ns):
    """MGP.end_to_end with tsne.tsne in place of PCA: the fixture's anomalous windows (the same scan, forced threshold and
    symmetric counts), np.random.seed(0) then tsne.tsne(anomCounts, 2, 50, 20.0) (the CLI's defaults, --seed 0), DBSCAN at an
    eps chosen as MGP.end_to_end chooses it, kept only if four perturbed starts give the same labels."""
    import pandas as pd
    import shutil
    import tempfile
    from sklearn.cluster import DBSCAN
    fa = os.path.join(INP, MGP.FASTA)
    m, k, w, inc, pmin, pmax, dims, perplexity = 1, 4, 200, 100, 1, 3, 2, 20.0
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
    anomLabels, anomCounts = np.array(names), np.vstack(counts)
    np.random.seed(0)
    Y0 = np.random.randn(anomCounts.shape[0], dims)
    Ys = [run_reference(T, anomCounts, Y0 * (1.0 + kk * PERTURB), dims, perplexity, trace=False)[0] for kk in range(5)]
    Y = Ys[0]
    dists = [np.sqrt(((Yk[:, None, :] - Yk[None, :, :]) ** 2).sum(-1))[np.triu_indices(len(Yk), 1)] for Yk in Ys]
    pair = dists[0]
    grid = np.geomspace(np.percentile(pair, 0.5), np.percentile(pair, 50), 400)

    def agreed(e):
        """the labels of every member at e, if they are all equal and no member has a pair distance within 1e-6 of e"""
        labs = [DBSCAN(eps=e, min_samples=MIN_SAMPLES).fit(Yk).labels_ for Yk in Ys]
        if all(np.array_equal(labs[0], lk) for lk in labs[1:]) and all(np.min(np.abs(dk - e)) > 1e-6 * e for dk in dists):
            return labs[0]
        return None
    labs = {}
    for e in grid:
        e = float("%.4g" % e)
        lab = agreed(e)
        if lab is not None and len(set(lab.tolist()) - {-1}) == 3:
            labs[e] = lab
    # as MGP.end_to_end: three clusters, some windows unclassified if such an eps exists (t-SNE may leave none)
    good = [e for e in labs if (labs[e] == -1).any()] or list(labs)
    assert good, "no eps gives three clusters on which the ensemble agrees"
    eps = good[len(good) // 2]
    y_pred = labs[eps]
    cluster_gff = "".join(ns["anomClust2gff"](ns["cluster2df"](Y, labels=anomLabels, y_pred=y_pred)))
    anomaly_gff = "".join(ns["anomaly2GFF"](anomWin, args))
    argv = ["-m", str(m), "-k", str(k), "-w", str(w), "-i", str(inc), "-F", repr(force), "--runProjection", "PY-TSNE",
            "--projectionDims", str(dims), "--pcaMin", str(pmin), "--pcaMax", str(pmax), "--cluster", "DBSCAN",
            "--epsDBSCAN", repr(eps), "--gffOutfile", "a.gff3"]
    return {"fasta": MGP.FASTA, "argv": argv, "forceThresholdKLD": force, "epsDBSCAN": eps, "n_windows": len(rows),
            "n_anomalous": len(names), "n_noise": int(np.sum(y_pred == -1)), "clusters": len(set(y_pred.tolist()) - {-1}),
            "cluster_gff_name": "PY-TSNE_DBSCAN_k_2_cluster_labeled_windows_a.gff3", "cluster_gff": cluster_gff,
            "anomaly_gff": anomaly_gff}


def main():
    MGP._patch_pandas()
    if os.path.isdir(ARR):
        for f in os.listdir(ARR):
            if f.endswith(".npz"):
                os.remove(os.path.join(ARR, f))
    os.makedirs(ARR, exist_ok=True)
    T = load_tsne()
    logging.getLogger().setLevel(logging.INFO)
    _memo_pca(T)
    cases = {}
    for seed, c in enumerate(CASES):
        cases[c[0]] = make_case(T, 100 + 10 * seed, *c)
        g = cases[c[0]]
        print("%-11s n %4d F %4d d %d perplexity %4.1f: tries <= %2d, eps %s, %d clusters, %d noise, final costs %s"
              % (c[0], g["n"], g["F"], g["dims"], g["perplexity"], g["tries_max"], g["eps"], g["clusters"], g["noise"],
                 ["%.4f" % v for v in g["ensemble_final_cost"]]), flush=True)
    ns = MG.load_reference_functions(extra=("getBEDSeq", "cluster2df", "anomClust2gff"))
    e2e = end_to_end(T, ns)
    print("e2e: %d anomalous windows, eps %s, %d clusters, %d noise" % (e2e["n_anomalous"], e2e["epsDBSCAN"], e2e["clusters"],
                                                                       e2e["n_noise"]))
    doc = {"min_samples": MIN_SAMPLES, "perturbation": PERTURB, "cases": cases, "e2e": e2e}
    with open(os.path.join(GOLD, "tsne.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    logging.disable(logging.NOTSET)
    main()
