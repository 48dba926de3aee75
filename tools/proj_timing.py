#!/usr/bin/env python3
"""Timings of the projection / clustering step on the GPU (frisk_amd.projection), printed as one JSON line.

  covariance, eigh (torch.linalg.eigh on the device) and transform ms at n = 30 000 and 100 000 windows of F = 2 772 features
  (--pcaMin 1 --pcaMax 6), and the covariance call's FP64 rate (2 n F^2 FLOP over its time; the kernels do half of that, the upper triangle);
  DBSCAN ms at n = 1e5 and 1e6 points of d = 2; k-means ms (k = 2, 20 starts) at n = 1e6;
  numpy / sklearn on the host's CPUs for the same work (null where sklearn is absent);
  PY-TSNE (exact t-SNE, d = 2, perplexity 20) at n = 5 000, 20 000 and 50 000 windows of F = 2 772 reduced to 50 columns:
  PCA-step, affinity and per-iteration ms, the 1000-iteration total, and the numpy restatement's ms per iteration on the host
  (tests/tsne_oracle.py, 20 iterations at n = 5 000);
  MDS (--mds-only, metric SMACOF, d = 2) at n = 5 000, 20 000 and 50 000 windows of F = 2 772: dissimilarity ms (the handle's
  create), ms per SMACOF step, iterations per start and the whole 5-start mds() ms; sklearn's MDS on the host at n = 2 000 and
  5 000 (--no-gpu: only those); written to --out as well as printed;
  IncrementalPCA (--ipca-only, d = 2, batches of 5 F = 13 860 rows) at n = 30 000 and 100 000 windows of F = 2 772: the whole
  incremental_pca() call and its split (statistics + Gram with the batch's copies, eigh, transform; device events around the
  statistics + stack kernels and around the Gram kernels), pca() on the same X, and sklearn's IncrementalPCA on the host at the
  --ipca-cpu-ns sizes; written to --out as well as printed.

Every GPU time is a host clock around one call, which ends in a device-to-host copy (so it includes the host-to-device copy of the
input); each shape is run once untimed first.  --small: tiny sizes, for a profiler run.

    python tools/proj_timing.py [--small] [--no-cpu] [--tsne-only]
    python tools/proj_timing.py --mds-only [--ns 5000 20000] [--no-cpu | --no-gpu] [--out profiles/proj/mds_timing.json]
    python tools/proj_timing.py --ipca-only [--ns 30000 100000] [--ipca-cpu-ns 30000] [--no-cpu] [--out profiles/proj/ipca_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _proportions(n, f, seed):
    rs = np.random.RandomState(seed)
    X = rs.gamma(0.5, size=(n, f)) * (1.0 + 3.0 * rs.uniform(size=f))
    return X / X.sum(axis=1, keepdims=True)


def _points(n, seed):
    rs = np.random.RandomState(seed)
    centres = np.array([(0.0, 0.0), (6.0, 0.0), (3.0, 5.0)])
    Y = centres[rs.randint(0, 3, size=n)] + rs.normal(size=(n, 2))
    return Y


def _ms(fn, *a, **k):
    t0 = time.perf_counter()
    out = fn(*a, **k)
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--tsne-only", action="store_true", help="only the PY-TSNE legs")
    ap.add_argument("--mds-only", action="store_true", help="only the MDS legs")
    ap.add_argument("--ipca-only", action="store_true", help="only the IncrementalPCA legs")
    ap.add_argument("--ipca-cpu-ns", type=int, nargs="+", default=None, help="with --ipca-only: the sizes of sklearn's runs on the host")
    ap.add_argument("--no-gpu", action="store_true", help="with --mds-only: only sklearn on the host")
    ap.add_argument("--ns", type=int, nargs="+", default=None, help="with --mds-only: the GPU sizes")
    ap.add_argument("--out", default=None, help="with --mds-only: also write the JSON here")
    opts = ap.parse_args()
    if opts.mds_only:
        doc = json.dumps({"tool": "proj_timing", "mds": mds_legs(opts)})
        print(doc)
        if opts.out:
            with open(opts.out, "w") as fh:
                fh.write(doc + "\n")
        return
    if opts.ipca_only:
        doc = json.dumps({"tool": "proj_timing", "ipca": ipca_legs(opts)})
        print(doc)
        if opts.out:
            with open(opts.out, "w") as fh:
                fh.write(doc + "\n")
        return
    if opts.tsne_only:
        print(json.dumps({"tool": "proj_timing", "tsne": tsne_legs(opts)}))
        return
    from frisk_amd import projection as P
    F = 2772
    pca_ns = (3000,) if opts.small else (30000, 100000)
    db_ns = (20000,) if opts.small else (100000, 1000000)
    km_n = 20000 if opts.small else 1000000
    eps = 0.05
    out = {"tool": "proj_timing", "F": F, "pca": {}, "dbscan": {"eps": eps, "d": 2}, "kmeans": {"k": 2, "n_init": 20}, "cpu": {}}
    for n in pca_ns:
        X = _proportions(n, F, n)
        P.pca(X, 2)                                                   # warm-up of the shape
        r = P.pca(X, 2)
        t = r.timings
        out["pca"][str(n)] = {"cov_ms": t["cov_ms"], "eigh_ms": t["eigh_ms"], "transform_ms": t["transform_ms"],
                              "cov_fp64_tflops": 2.0 * n * F * F / (t["cov_ms"] * 1e-3) / 1e12}
        if not opts.no_cpu:
            def np_cov(X=X):
                Xc = X - X.mean(axis=0)
                return (Xc.T @ Xc) / (X.shape[0] - 1)
            out["cpu"]["numpy_cov_ms_%d" % n] = _ms(np_cov)[0]
            if "numpy_eigh_ms" not in out["cpu"]:
                _, c = P.cov(X)
                out["cpu"]["numpy_eigh_ms"] = _ms(np.linalg.eigh, c)[0]
    for n in db_ns:
        Y = _points(n, n)
        P.dbscan(Y, eps)
        ms, lab = _ms(P.dbscan, Y, eps)
        out["dbscan"][str(n)] = {"ms": ms, "clusters": int(lab.max()) + 1, "noise": int((lab == -1).sum())}
    Y = _points(km_n, 7)
    P.kmeans(Y, 2, seed=0)
    ms, r = _ms(P.kmeans, Y, 2, seed=0)
    out["kmeans"][str(km_n)] = {"ms": ms, "inertia": r.inertia, "n_iter_best": r.n_iter}
    if not opts.no_cpu:
        try:
            from sklearn.cluster import DBSCAN, KMeans
            Yd = _points(db_ns[0], db_ns[0])
            out["cpu"]["sklearn_dbscan_ms_%d" % db_ns[0]] = _ms(lambda: DBSCAN(eps=eps, min_samples=50).fit(Yd))[0]
            out["cpu"]["sklearn_kmeans_ms_%d" % km_n] = _ms(lambda: KMeans(2, n_init=20, max_iter=500, tol=1e-4,
                                                                            random_state=0).fit(Y))[0]
        except ImportError:
            out["cpu"]["sklearn"] = None
    out["cpu"]["threads"] = os.cpu_count()
    out["tsne"] = tsne_legs(opts)
    print(json.dumps(out))


def tsne_legs(opts):
    from frisk_amd import projection as P
    F, iters = 2772, P.TSNE_ITERATIONS
    out = {"F": F, "initial_dims": 50, "d": 2, "perplexity": 20.0, "iterations": iters}
    for n in ((1000,) if opts.small else (5000, 20000, 50000)):
        X = _proportions(n, F, n)
        t0 = time.perf_counter()
        Xp = P.tsne_input(X, 50)
        t1 = time.perf_counter()
        with P.TSNE(Xp, np.random.RandomState(0).randn(n, 2), 20.0) as h:
            t1c = time.perf_counter()
            beta, tries = h.affinities()
            t2 = time.perf_counter()
            h.run(0, 10)                  # warm-up of the iteration kernels (counted in the total below)
            t3 = time.perf_counter()
            cost = h.run(10, iters)
            t4 = time.perf_counter()
        out[str(n)] = {"pca_step_ms": 1e3 * (t1 - t0), "create_ms": 1e3 * (t1c - t1), "affinity_ms": 1e3 * (t2 - t1c), "tries_mean": float(tries.mean()),
                       "tries_max": int(tries.max()), "ms_per_iteration": 1e3 * (t4 - t3) / (iters - 10),
                       "iterations_total_ms": 1e3 * (t4 - t2), "final_cost": float(cost[-1])}
    if not opts.no_cpu:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
        import tsne_oracle as TO
        n = 1000 if opts.small else 5000
        Xp = P.tsne_input(_proportions(n, F, n), 50)
        _b, _t, q = TO.affinities(Xp, 20.0)
        Y, iY, gains = np.random.RandomState(0).randn(n, 2), np.zeros((n, 2)), np.ones((n, 2))
        t0 = time.perf_counter()
        for t in range(20):
            st = TO.step(Y, iY, gains, q, t)
            Y, iY, gains = st.Y, st.iY, st.gains
        out["numpy_oracle_ms_per_iteration_%d" % n] = 1e3 * (time.perf_counter() - t0) / 20
    return out


def mds_legs(opts):
    F = 2772
    out = {"F": F, "d": 2, "n_init": 5, "max_iter": 500, "eps": 1e-3}
    if not opts.no_gpu:
        from frisk_amd import projection as P
        P.mds(_proportions(300, F, 1), 2)           # first launches
        for n in opts.ns or ((1000,) if opts.small else (5000, 20000, 50000)):
            X = _proportions(n, F, n)
            Y0 = np.random.RandomState(0).uniform(size=(n, 2))
            t0 = time.perf_counter()
            with P.MDS(X, 2) as h:
                t1 = time.perf_counter()
                h.run(Y0, 1, 0.0)                   # 2 passes
                t2 = time.perf_counter()
                h.run(Y0, 21, 0.0)                  # 22 passes
                t3 = time.perf_counter()
            r = P.mds(X, 2)
            out[str(n)] = {"dissimilarities_ms": 1e3 * (t1 - t0), "ms_per_step": 1e3 * ((t3 - t2) - (t2 - t1)) / 20,
                           "n_iters": r.n_iters, "best_start": r.best_start, "stress": r.stress, "mds_ms": sum(r.timings.values()),
                           "mds_timings": r.timings, "D_floor_ms_per_step": 8.0 * n * n / 6.3e12 * 1e3}
    if not opts.no_cpu:
        from sklearn.manifold import MDS
        for n in ((500,) if opts.small else (2000, 5000)):
            X = _proportions(n, F, n)
            m = MDS(n_components=2, metric=True, n_init=5, max_iter=500, eps=1e-3, n_jobs=1, random_state=0,
                    dissimilarity="euclidean", normalized_stress=False)
            ms, _ = _ms(m.fit_transform, X)
            out["sklearn_%d" % n] = {"ms": ms, "n_iter": int(m.n_iter_), "threads": os.cpu_count()}
    return out


def _blobs(n, f, seed):
    """Three blobs of proportions (a PCA of structureless rows has no leading components to time a projection on)."""
    rs = np.random.RandomState(seed)
    centres = rs.dirichlet(np.full(f, 2.0), size=3)
    X = rs.standard_gamma(centres[rs.randint(0, 3, n)] * 200.0 + 1e-3)
    return X / X.sum(axis=1, keepdims=True)


def ipca_legs(opts):
    from frisk_amd import projection as P
    F, d = 2772, 2
    out = {"F": F, "d": d, "batch_size": 5 * F}
    ns = opts.ns or ((3000,) if opts.small else (30000, 100000))
    P.incremental_pca(_blobs(300, F, 1), d)         # first launches
    for n in ns:
        X = _blobs(n, F, n)
        P.incremental_pca(X[:min(n, 2 * 5 * F + 7)], d)             # warm-up of the batch shapes
        ms, r = _ms(P.incremental_pca, X, d)
        t = r.timings
        P.pca(X, d)
        pms, pr = _ms(P.pca, X, d)
        out[str(n)] = {"batches": r.batch_sizes, "incremental_pca_ms": ms, "stats_gram_ms": t["stats_gram_ms"], "eigh_ms": t["eigh_ms"],
                       "transform_ms": t["transform_ms"], "stats_stack_kernels_ms": t["stats_kernels_ms"],
                       "gram_kernels_ms": t["gram_kernels_ms"], "eigh_share": t["eigh_ms"] / ms,
                       "gram_kernels_fp64_tflops": 2.0 * n * F * F / (t["gram_kernels_ms"] * 1e-3) / 1e12,
                       "explained_variance": r.explained_variance_.tolist(), "pca_ms": pms, "pca_timings": pr.timings}
    if not opts.no_cpu:
        from sklearn.decomposition import IncrementalPCA
        for n in opts.ipca_cpu_ns or ns:
            X = _blobs(n, F, n)
            m = IncrementalPCA(n_components=d, whiten=False, copy=True, batch_size=None)
            ms, _ = _ms(lambda: m.fit(X).transform(X))
            out["sklearn_%d" % n] = {"ms": ms, "threads": os.environ.get("OMP_NUM_THREADS") or os.cpu_count()}
    return out


if __name__ == "__main__":
    main()
