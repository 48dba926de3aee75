#!/usr/bin/env python3
"""Goldens of the projection / clustering step (reference L1556-1697): tests/golden/projection_cluster.json (parameters, labels of
the writer cases, GFF3 texts), the arrays it names under tests/golden/projection_cluster/ (.npy: inputs, sklearn's outputs, labels)
and the fixture FASTA tests/golden/inputs/proj_islands.fa.

Everything here comes from the reference's own functions (tools/make_golden.load_reference_functions) and sklearn: PCA with
svd_solver="full", DBSCAN(min_samples=50) and KMeans(n_init=20, max_iter=500, tol=1e-4, random_state=0).  This script does
not use the package under test.  Every random input is drawn from a fixed numpy RandomState, so a rerun writes the same bytes.
The edge goldens (keys dbscan_edges, kmeans_init, kmeans_more, pca_large) also use the numpy restatements of tests/proj_oracles.py
to keep only cases whose decisions the kernels can reproduce exactly.

    python tools/make_golden_projection.py
"""
import json
import os
import sys
import warnings

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # sklearn's k-means sums in thread chunks: one thread, one order, the same last bits every run
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import proj_oracles as PO  # noqa: E402     numpy restatements shared with the tests (no package code)

GOLD, INP = MG.GOLD, MG.INP
ARR = os.path.join(GOLD, "projection_cluster")
FASTA = "proj_islands.fa"
MIN_SAMPLES = 50


def _patch_pandas():
    """pandas of the reference's day: DataFrame.as_matrix and df[['col']] = Series (as make_golden.run_writers)."""
    import pandas as pd
    warnings.simplefilter("ignore")
    pd.options.mode.chained_assignment = None
    if not hasattr(pd.DataFrame, "as_matrix"):
        pd.DataFrame.as_matrix = lambda self, columns=None: (self[columns] if columns is not None else self).values
    orig = pd.DataFrame.__setitem__

    def old_setitem(self, key, value):
        if isinstance(key, list) and len(key) == 1 and isinstance(value, pd.Series):
            key = key[0]
        return orig(self, key, value)
    pd.DataFrame.__setitem__ = old_setitem


def _arr(key, a, dtype=np.float64):
    """Save one array as <key>.npy under ARR (the .npy format has no timestamp: a rerun writes the same bytes); the JSON holds
    its file name."""
    name = key + ".npy"
    np.save(os.path.join(ARR, name), np.ascontiguousarray(a, dtype=dtype))
    return name


# ------------------------------------------------------------------------------------------------ fixture FASTA
def write_fixture():
    """Two scaffolds of uniform background with islands of three compositions (A/T-rich, G/C-rich, A/G-rich), each island a
    multiple of the window step long and placed on a multiple of it."""
    rs = np.random.RandomState(20261015)
    comps = {"AT": [0.4, 0.4, 0.1, 0.1], "GC": [0.1, 0.1, 0.4, 0.4], "AG": [0.4, 0.1, 0.4, 0.1]}
    layout = {"chrP1": (22000, [(2000, "AT"), (7000, "GC"), (12000, "AG"), (17000, "AT")]),
              "chrP2": (18000, [(1000, "GC"), (5500, "AG"), (10000, "AT"), (14500, "GC"), (16000, "AG")])}
    island = 2500
    out = []
    for name, (length, isl) in layout.items():
        seq = rs.choice(list("ATGC"), size=length, p=[0.25] * 4)
        for start, comp in isl:
            n = min(island, length - start)
            seq[start:start + n] = rs.choice(list("ATGC"), size=n, p=comps[comp])
        text = "".join(seq.tolist())
        out.append(">" + name + "\n" + "\n".join(text[i:i + 100] for i in range(0, len(text), 100)) + "\n")
    with open(os.path.join(INP, FASTA), "w") as fh:
        fh.write("".join(out))


# ------------------------------------------------------------------------------------------------ unit goldens
def pca_cases():
    from sklearn.decomposition import PCA
    rs = np.random.RandomState(7)
    out = {}
    for name, n, f, d, scales in (("pca_n120_f8_d2", 120, 8, 2, [9.0, 4.0, 1.0]), ("pca_n160_f24_d3", 160, 24, 3, [12.0, 6.0, 3.0, 1.0])):
        q, _ = np.linalg.qr(rs.normal(size=(f, f)))
        z = rs.normal(size=(n, f)) * 0.05
        z[:, :len(scales)] = rs.normal(size=(n, len(scales))) * np.array(scales)
        X = (z @ q.T) * 0.01 + rs.uniform(0.0, 0.2, size=f)        # proportions-like: small values around a positive mean
        p = PCA(n_components=d, svd_solver="full").fit(X)
        out[name] = {"d": d, "X": _arr(name + ".X", X), "Y": _arr(name + ".Y", p.transform(X)),
                     "components": _arr(name + ".components", p.components_),
                     "explained_variance": _arr(name + ".explained_variance", p.explained_variance_), "mean": _arr(name + ".mean", p.mean_)}
    return out


def dbscan_cases():
    from sklearn.cluster import DBSCAN
    rs = np.random.RandomState(11)
    cases = {}
    # integer grid, 12 copies of every point: interior points have 5 x 12 = 60 neighbours at distance <= 1 (ties at exactly
    # eps = 1.0, exact in floating point), edge points 48 and corners 36 (border points); two blocks and a stray point
    g = [(x, y) for x in range(6) for y in range(6)] * 12 + [(x + 10, y) for x in range(5) for y in range(4)] * 12 + [(30, 30)]
    grid = np.array(g, dtype=float)[rs.permutation(len(g))]
    cases["grid_eps1"] = (grid, 1.0)
    # a border point (1, 0) within eps of a core point of two clusters; the cluster of the smaller seed index (B) must get it
    b = [(2.0, 0.0)] + [(3.0, 0.0)] * 55
    a = [(0.0, 0.0)] + [(-1.0, 0.0)] * 55
    cases["shared_border"] = (np.array(b + a + [(1.0, 0.0), (1.0, 5.0)]), 1.0)
    cases["all_noise"] = (rs.uniform(0.0, 100.0, size=(40, 2)), 1.0)
    blobs = np.vstack([rs.normal(c, 0.3, size=(m, 3)) for c, m in ((0.0, 120), (4.0, 90), (8.0, 40))] + [rs.uniform(-3, 11, size=(15, 3))])
    cases["blobs_d3"] = (blobs, 0.6)
    out = {}
    for name, (Y, eps) in cases.items():
        lab = DBSCAN(eps=eps, min_samples=MIN_SAMPLES).fit(Y).labels_
        out[name] = {"eps": eps, "Y": _arr("dbscan_" + name + ".Y", Y), "labels": _arr("dbscan_" + name + ".labels", lab, np.int32)}
    return out


def kmeans_cases():
    from sklearn.cluster import KMeans
    rs = np.random.RandomState(13)
    out = {}
    for name, centres, k in (("blobs_k3", [(0, 0), (6, 1), (2, 7)], 3), ("blobs_k2", [(0, 0, 0), (5, 5, 5)], 2)):
        Y = np.vstack([rs.normal(c, 0.7, size=(150 + 25 * i, len(c))) for i, c in enumerate(centres)])
        Y = Y[rs.permutation(len(Y))]
        km = KMeans(n_clusters=k, n_init=20, max_iter=500, tol=1e-4, random_state=0).fit(Y)
        out[name] = {"k": k, "inertia": float(km.inertia_), "Y": _arr("kmeans_" + name + ".Y", Y),
                     "labels": _arr("kmeans_" + name + ".labels", km.labels_, np.int32)}
    return out


# ------------------------------------------------------------------------------------------------ edge goldens
def _embed(rs, d, vec):
    """vec (length <= d) spread over d dimensions at random positions"""
    out = np.zeros(d)
    out[rs.permutation(d)[:len(vec)]] = vec
    return out


def dbscan_edge_cases():
    """Integer-coordinate DBSCAN cases at d = 5, 16, 17 and 64 (every instantiation of db_pairs past MAXD = 4; sklearn takes its
    brute-force path for d > 15), where every squared distance is an exact small integer, so a tie at eps is a tie in sklearn and
    in the kernel alike:
      ties_<d>     two core groups that reach one another only through Pythagorean offsets of length exactly eps (3-4-5 with
                   eps = 5, 1-2-2-3 with eps = 3) and a border point at exactly eps from a core point of each of two clusters;
      blobs_<d>    integer blobs with jitter in {-2..2}: many pairs at exactly eps, noise between;
      noise_<d>    points at pairwise distance > eps: every label -1."""
    from sklearn.cluster import DBSCAN
    rs = np.random.RandomState(29)
    cases = {}
    for d in (5, 16, 17, 64):
        for name, o, eps in (("ties345", (3.0, 4.0), 5.0), ("ties1223", (1.0, 2.0, 2.0), 3.0)):
            O = rs.randint(-50, 50, size=d).astype(float)
            o = _embed(rs, d, o)
            axis = np.zeros(d)                                  # a unit axis orthogonal to o
            free = [q for q in range(d) if o[q] == 0.0]
            axis[free[rs.randint(len(free))]] = 1.0
            # core a0 = O with tails O - j axis (j = 1..3), core c0 = O + 2 o with tails c0 - j axis; border X = O + o at exactly
            # eps from a0 and from c0 and farther than eps from every tail point
            grpC = [O + 2 * o] + [O + 2 * o - j * axis for j in (1, 2, 3)]
            grpA = [O] + [O - j * axis for j in (1, 2, 3)]
            X = O + o
            far = [O + 40.0 * j * axis + _embed(rs, d, rs.randint(-2, 3, size=3).astype(float)) for j in range(1, 7)]
            Y = np.array(grpC + [X] + grpA + far)
            cases["%s_d%d" % (name, d)] = (Y, eps, 4)
        centres = [rs.randint(-30, 30, size=d) * 3 for _ in range(3)]
        pts = np.vstack([c + rs.randint(-2, 3, size=(m, d)) for c, m in zip(centres, (70, 50, 30))] +
                        [rs.randint(-120, 120, size=(12, d))]).astype(float)
        pts = pts[rs.permutation(len(pts))]
        sq = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
        eps = float(np.floor(np.sqrt(np.percentile(sq[sq > 0], 15))))    # an integer eps inside the blobs: many pairs tie at it
        cases["blobs_d%d" % d] = (pts, eps, 10)
        cases["noise_d%d" % d] = (np.array([rs.randint(-3, 4, size=d) + 100 * j for j in range(20)], dtype=float), 5.0, 2)
    out = {}
    for name, (Y, eps, ms) in cases.items():
        sq = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
        assert np.array_equal(Y, np.round(Y)) and np.abs(Y).max() < 2 ** 20        # integer data: every distance decision exact
        lab = DBSCAN(eps=eps, min_samples=ms).fit(Y).labels_
        want, _gap = PO.dbscan_oracle(Y, eps, ms)
        assert np.array_equal(lab, want), name
        if name.startswith("ties"):
            assert (sq == eps * eps).any() and (lab[:5] == 0).all() and (lab[5:9] == 1).all() and (lab[9:] == -1).all(), name
        if name.startswith("noise"):
            assert (lab == -1).all(), name
        out[name] = {"eps": eps, "min_samples": ms, "Y": _arr("dbscan_" + name + ".Y", Y),
                     "labels": _arr("dbscan_" + name + ".labels", lab, np.int32)}
    return out


def _stale_lloyd(Y, C0, max_iter, tol):
    """the pre-relocation rule (an empty cluster keeps its centre): used only to keep cases that tell the two rules apart"""
    C = np.array(C0, dtype=float)
    old = np.full(len(Y), -1)
    for _ in range(max_iter):
        lab = np.argmin(PO.sq_dist(Y, C), axis=1)
        Cn = C.copy()
        for c in range(len(C)):
            if (lab == c).any():
                Cn[c] = Y[lab == c].mean(axis=0)
        shift, C = float(np.sum((Cn - C) ** 2)), Cn
        if np.array_equal(lab, old) or shift <= tol:
            break
        old = lab
    return np.argmin(PO.sq_dist(Y, C), axis=1), C


def _sk_tol(Y, tol):
    return float(np.mean(np.var(Y, axis=0)) * tol)        # sklearn's _tolerance


def kmeans_init_cases():
    """KMeans(init=C0, n_init=1, max_iter=500, tol=1e-4) from explicit centres: clusters that go empty mid-run (one per step with
    a unique farthest point, and two in one step), points duplicated at fewer than k locations (no relocation: the largest
    distance is 0), d = 5, 17 and 64, k = 1 and k = n.  A case is kept only where PO.lloyd (the kernel's rule restated) gives
    sklearn's labels and n_iter_; the relocation cases also only where the pre-relocation rule ends elsewhere."""
    from sklearn.cluster import KMeans
    cases = {}
    one, two = [], []
    for seed in range(4000):
        if len(one) >= 2 and len(two) >= 1:
            break
        rs = np.random.RandomState(seed)
        n, k = rs.randint(20, 41), rs.randint(4, 7)
        Y = rs.uniform(0.0, 10.0, size=(n, 2))
        C0 = rs.uniform(-2.0, 12.0, size=(k, 2))
        trace = []
        lab, C, _, _ = PO.lloyd(Y, C0, 500, _sk_tol(Y, 1e-4), trace)
        steps = [t for t in trace if t["moved"]]
        if not steps or not all(t["unique_far"] for t in trace):
            continue
        slab, sC = _stale_lloyd(Y, C0, 500, _sk_tol(Y, 1e-4))
        if np.array_equal(slab, lab) and np.allclose(sC, C):
            continue
        if all(t["empty"] == 1 for t in trace if t["empty"]) and len(one) < 2:
            one.append((seed, Y, C0))
        elif any(t["empty"] == 2 and len(t["moved"]) == 2 for t in trace) and not two:
            two.append((seed, Y, C0))
    assert len(one) == 2 and len(two) == 1
    for j, (seed, Y, C0) in enumerate(one):
        cases["empty_one_%d" % j] = (Y, C0)
    cases["empty_two"] = (two[0][1], two[0][2])
    # duplicates at two locations, k = 4: clusters stay empty and are placed on the largest cluster a - its centre when a comes
    # first in id order, its coordinate sum when it comes after (sklearn's _average_centers).  sklearn runs on X - mean(X): the
    # column means here are exact binary fractions (so every distance to a centre is exactly 0), and 0 in the second case (so
    # that sklearn's sum of centred coordinates is the plain sum).
    cases["dups_after"] = (np.array([(0.0, 0.0)] * 6 + [(4.0, 8.0)] * 2), np.array([(0.0, 0.0), (4.0, 8.0), (5.0, 5.0), (-4.0, 2.0)]))
    cases["dups_before"] = (np.array([(1.0, 2.0)] * 6 + [(-2.0, -4.0)] * 3), np.array([(5.0, 5.0), (-2.0, -4.0), (1.0, 2.0), (-4.0, 2.0)]))
    rs = np.random.RandomState(31)
    for d in (5, 17, 64):
        Y = np.vstack([rs.normal(rs.uniform(-4, 4, size=d), 1.0, size=(m, d)) for m in (90, 70, 50, 40)])
        Y = Y[rs.permutation(len(Y))]
        cases["d%d" % d] = (Y, Y[rs.choice(len(Y), 4, replace=False)] + rs.normal(0, 0.5, size=(4, d)))
    Y = rs.normal(size=(50, 3))
    cases["k1"] = (Y, rs.normal(size=(1, 3)))
    Y = rs.uniform(0, 5, size=(12, 2))
    cases["kn"] = (Y, Y[rs.permutation(12)] + rs.normal(0, 1e-3, size=(12, 2)))
    out = {}
    for name, (Y, C0) in cases.items():
        tol = _sk_tol(Y, 1e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km = KMeans(n_clusters=len(C0), init=C0, n_init=1, max_iter=500, tol=1e-4).fit(Y)
        lab, C, inertia, it = PO.lloyd(Y, C0, 500, tol)
        assert np.array_equal(lab, km.labels_) and it == km.n_iter_, name
        assert np.allclose(C, km.cluster_centers_, rtol=1e-12, atol=1e-12 * np.abs(Y).max()), name
        assert abs(inertia - km.inertia_) <= 1e-12 * max(km.inertia_, 1.0), name
        key = "kminit_" + name
        out[name] = {"k": len(C0), "tol": tol, "max_iter": 500, "inertia": float(km.inertia_), "n_iter": int(km.n_iter_),
                     "Y": _arr(key + ".Y", Y), "init": _arr(key + ".init", C0), "labels": _arr(key + ".labels", km.labels_, np.int32),
                     "centers": _arr(key + ".centers", km.cluster_centers_)}
    return out


def kmeans_more_cases():
    """KMeans(n_init=20, max_iter=500, tol=1e-4, random_state=0) (k-means++ seeding) at d = 5 and d = 17, as kmeans_cases."""
    from sklearn.cluster import KMeans
    rs = np.random.RandomState(37)
    out = {}
    for name, d, k in (("blobs_d5_k4", 5, 4), ("blobs_d17_k3", 17, 3)):
        Y = np.vstack([rs.normal(rs.uniform(-6, 6, size=d), 1.0, size=(120 + 30 * i, d)) for i in range(k)])
        Y = Y[rs.permutation(len(Y))]
        km = KMeans(n_clusters=k, n_init=20, max_iter=500, tol=1e-4, random_state=0).fit(Y)
        out[name] = {"k": k, "inertia": float(km.inertia_), "Y": _arr("kmeans_" + name + ".Y", Y),
                     "labels": _arr("kmeans_" + name + ".labels", km.labels_, np.int32)}
    return out


def pca_large_cases():
    """PCA(n_components=d, svd_solver="full") at F = 2 772 (--pcaMin 1 --pcaMax 6) on PO.planted_pca_input: X is not stored, its
    seed and sha256 are; eigengap = (lambda_d - lambda_(d+1)) / lambda_1 scales the tests' tolerances."""
    from sklearn.decomposition import PCA
    out = {}
    for n in (300, 3000):
        for d in (2, 5):
            seed = 1000 + n + d
            X = PO.planted_pca_input(n, d, seed)
            p = PCA(n_components=d + 1, svd_solver="full").fit(X)
            ev = p.explained_variance_
            name = "pca_n%d_f%d_d%d" % (n, X.shape[1], d)
            out[name] = {"n": n, "f": X.shape[1], "d": d, "seed": seed, "sha256": PO.sha256(X),
                         "eigengap": float((ev[d - 1] - ev[d]) / ev[0]),
                         "Y": _arr(name + ".Y", p.transform(X)[:, :d]), "components": _arr(name + ".components", p.components_[:d]),
                         "explained_variance": _arr(name + ".explained_variance", ev[:d])}
    return out


def writer_cases(ns):
    rs = np.random.RandomState(17)
    labels = np.array([["chr%s:%d:%d" % ("AB"[i % 2], 1 + 250 * i, 500 + 250 * i)] for i in range(12)])
    Y = rs.normal(size=(12, 2))
    out = {}
    for name, y in (("noise", [1, -1, 0, 0, 2, -1, 1, 2, 0, 1, -1, 2]), ("no_noise", [2, 0, 1, 1, 0, 2, 2, 0, 1, 0, 1, 2])):
        df = ns["cluster2df"](Y, labels=labels, y_pred=np.array(y))
        out[name] = {"labels": labels[:, 0].tolist(), "y_pred": y, "gff": "".join(ns["anomClust2gff"](df))}
    return out


# ------------------------------------------------------------------------------------------------ end to end
class _Args:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def end_to_end(ns):
    """The reference's main() from the window scores to the two GFF3 files, on the fixture: scan (L1478-1494), forced threshold,
    thresholdKLD(merge=False), symmetric counts (L1571-1591), PCA (L1612), DBSCAN (L1639), cluster2df + anomClust2gff (L1697),
    anomaly2GFF of the recycled windows (L1672-1686)."""
    import pandas as pd
    from sklearn.cluster import DBSCAN
    from sklearn.decomposition import PCA
    fa = os.path.join(INP, FASTA)
    m, k, w, inc, pmin, pmax, dims = 1, 4, 200, 100, 1, 3, 2
    import shutil
    import tempfile
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
    # forced threshold in the middle of the widest gap of log10(KLD) above the median, so that no window is near the cut
    lk = np.sort(np.log10(allWindows["windowKLD"].values))
    hi = lk[len(lk) // 2:]
    j = int(np.argmax(np.diff(hi)))
    force = float("%.4g" % 10 ** ((hi[j] + hi[j + 1]) / 2))
    args = _Args(findSelf=False, mergeDist=0, dimReduce="windows", forceThresholdKLD=force, threshTypeKLD=None, percentileKLD=99.0,
                 pcaMin=pmin, pcaMax=pmax, minWordSize=m, maxWordSize=k, maskHost=False, hostSeq=None, windowlen=w)
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
    Y = PCA(n_components=dims).fit(anomCounts).transform(anomCounts)
    # eps: the middle of the range of eps that gives three clusters; no pair distance within 1e-6 of it (relative)
    dist = np.sqrt(((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1))
    pair = dist[np.triu_indices(len(Y), 1)]
    grid = np.geomspace(np.percentile(pair, 0.5), np.percentile(pair, 50), 400)
    # (among those, the ones that leave some windows unclassified: the writer's Unclassified / Class_1 naming is exercised)
    labs = {e: DBSCAN(eps=e, min_samples=MIN_SAMPLES).fit(Y).labels_ for e in grid}
    good = [e for e in grid if len(set(labs[e].tolist()) - {-1}) == 3 and (labs[e] == -1).any()]
    assert good, "no eps gives three clusters and noise"
    eps = float("%.4g" % good[len(good) // 2])
    assert np.min(np.abs(pair - eps)) > 1e-6 * eps
    y_pred = DBSCAN(eps=eps, min_samples=MIN_SAMPLES).fit(Y).labels_
    cluster_gff = "".join(ns["anomClust2gff"](ns["cluster2df"](Y, labels=anomLabels, y_pred=y_pred)))
    anomaly_gff = "".join(ns["anomaly2GFF"](anomWin, args))
    argv = ["-m", str(m), "-k", str(k), "-w", str(w), "-i", str(inc), "-F", repr(force), "--runProjection", "PCA",
            "--projectionDims", str(dims), "--pcaMin", str(pmin), "--pcaMax", str(pmax), "--cluster", "DBSCAN",
            "--epsDBSCAN", repr(eps), "--gffOutfile", "a.gff3"]
    return {"fasta": FASTA, "argv": argv, "forceThresholdKLD": force, "epsDBSCAN": eps, "n_windows": len(rows),
            "n_anomalous": len(names), "n_noise": int(np.sum(y_pred == -1)), "labels": _arr("e2e.labels", anomLabels[:, 0], str),
            "y_pred": _arr("e2e.y_pred", y_pred, np.int32), "Y": _arr("e2e.Y", Y), "cluster_gff_name": "PCA_DBSCAN_k_2_cluster_labeled_windows_a.gff3",
            "cluster_gff": cluster_gff, "anomaly_gff": anomaly_gff}


def main():
    import sklearn
    _patch_pandas()
    if os.path.isdir(ARR):
        for f in os.listdir(ARR):
            if f.endswith(".npy"):
                os.remove(os.path.join(ARR, f))
    os.makedirs(ARR, exist_ok=True)
    write_fixture()
    ns = MG.load_reference_functions(extra=("getBEDSeq", "cluster2df", "anomClust2gff"))
    doc = {"sklearn": sklearn.__version__, "min_samples": MIN_SAMPLES, "pca": pca_cases(), "dbscan": dbscan_cases(),
           "kmeans": kmeans_cases(), "writers": writer_cases(ns), "e2e": end_to_end(ns),
           "dbscan_edges": dbscan_edge_cases(), "kmeans_init": kmeans_init_cases(), "kmeans_more": kmeans_more_cases(),
           "pca_large": pca_large_cases()}
    with open(os.path.join(GOLD, "projection_cluster.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    e = doc["e2e"]
    print("projection_cluster: %d windows, %d anomalous, clusters %s, eps %s, F %s"
          % (e["n_windows"], e["n_anomalous"], sorted(set(np.load(os.path.join(ARR, e["y_pred"])).tolist())), e["epsDBSCAN"],
             e["forceThresholdKLD"]))
    for name, c in doc["dbscan"].items():
        print("dbscan %-14s labels %s" % (name, sorted(set(np.load(os.path.join(ARR, c["labels"])).tolist()))))


if __name__ == "__main__":
    main()
