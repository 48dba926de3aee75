#!/usr/bin/env python3
"""Timings of the projection / clustering step on the GPU (frisk_amd.projection), printed as one JSON line.

  covariance, eigh (torch.linalg.eigh on the device) and transform ms at n = 30 000 and 100 000 windows of F = 2 772 features
  (--pcaMin 1 --pcaMax 6), and the covariance call's FP64 rate (2 n F^2 FLOP over its time; the kernels do half of that, the upper triangle);
  DBSCAN ms at n = 1e5 and 1e6 points of d = 2; k-means ms (k = 2, 20 starts) at n = 1e6;
  numpy / sklearn on the host's CPUs for the same work (null where sklearn is absent).

Every GPU time is a host clock around one call, which ends in a device-to-host copy (so it includes the host-to-device copy of the
input); each shape is run once untimed first.  --small: tiny sizes, for a profiler run.

    python tools/proj_timing.py [--small] [--no-cpu]
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
    opts = ap.parse_args()
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
