#!/usr/bin/env python3
"""Device time of the spectral kernels (csrc/spectral_kernels.h) and wall-clock of projection.spectral at n = 2 000 and 20 000
points, d = 2, k = 3 (three Gaussian blobs).  Each shape is run once to warm up, then once more with a host clock around each
call; the kernels are timed with the handle's HIP events.  A product reads M once, 8 n^2 bytes, so bytes / time is set against
the HBM rate (--hbm-gbs, 8000 for an MI355X) as the achieved fraction.  The host share of a step is the iteration's host linear
algebra (QR, Rayleigh-Ritz, residuals) over host + product wall-clock (the product's wall-clock includes the transfers of Q and
Z).  With --sklearn the same case runs through sklearn's SpectralClustering on the host's CPU, at the sizes up to --sklearn-max-n
(not part of the package; the only comparison there is).  Writes one JSON document (--out) and prints a markdown table (DESIGN.md
section 9.5).  Runs no test.

    python tools/spectral_timing.py [--n 2000 20000] [--sklearn] [--out profiles/spectral/spectral_timing.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))


def blobs(n, seed=7):
    rs = np.random.RandomState(seed)
    sizes = [n // 2, n // 3, n - n // 2 - n // 3]
    centres = [(0.0, 0.0), (5.0, 2.5), (10.0, 0.0)]
    return np.vstack([np.array(c) + 0.25 * rs.normal(size=(m, 2)) for c, m in zip(centres, sizes)])


def run(P, Y, k, device):
    t0 = time.perf_counter()
    r = P.spectral(Y, k, seed=0, device=device)
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-max-n", type=int, default=2000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("profiles", "spectral", "spectral_timing.json"))
    a = ap.parse_args()
    from frisk_amd import projection as P
    doc = {"d": 2, "k": a.k, "hbm_gbs": a.hbm_gbs, "shapes": []}
    for n in a.n:
        Y = blobs(n)
        run(P, Y, a.k, a.device)                                # warm-up of the whole path at this shape
        r, wall = run(P, Y, a.k, a.device)
        t = r.timings
        per_product = t["products_ms"] / r.n_iter
        res = {"n": n, "m_bytes": 8 * n * n, "affinity_ms": t["affinity_ms"], "normalise_ms": t["normalise_ms"],
               "product_ms": per_product, "product_hbm_fraction": 8.0 * n * n / (per_product * 1e-3) / (a.hbm_gbs * 1e9),
               "iterations": r.n_iter, "residual": float(r.residuals.max()), "product_wall_ms": t["products_wall_ms"] / r.n_iter,
               "host_ms_per_step": t["host_ms"] / r.n_iter, "host_share_of_step": t["host_ms"] / (t["host_ms"] + t["products_wall_ms"]),
               "embedding_ms": t["embedding_ms"], "kmeans_ms": t["kmeans_ms"], "wall_s": wall,
               "cluster_sizes": np.bincount(r.labels).tolist()}
        if a.sklearn and n <= a.sklearn_max_n:
            import warnings
            from sklearn.cluster import SpectralClustering
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                m = SpectralClustering(n_clusters=a.k, eigen_solver=None, random_state=0, n_init=20, gamma=1.0, affinity="rbf",
                                       eigen_tol=0.0, assign_labels="kmeans").fit(Y)
                res["sklearn_s"] = time.perf_counter() - t0
            res["sklearn_cpus"] = len(os.sched_getaffinity(0))
            seen, seen2 = {}, {}
            res["same_partition_as_sklearn"] = ([seen.setdefault(int(c), len(seen)) for c in m.labels_] ==
                                                [seen2.setdefault(int(c), len(seen2)) for c in r.labels])
        else:
            res["sklearn_s"] = None                             # not run at this size
        doc["shapes"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("| n | affinity ms | normalise ms | product ms | of the HBM rate | iterations | host share of a step | whole run s | sklearn s |")
    print("|---|---|---|---|---|---|---|---|---|")
    for s in doc["shapes"]:
        print("| %d | %.3f | %.3f | %.3f | %.2f | %d | %.2f | %.2f | %s |" % (
            s["n"], s["affinity_ms"], s["normalise_ms"], s["product_ms"], s["product_hbm_fraction"], s["iterations"],
            s["host_share_of_step"], s["wall_s"], "not run" if s["sklearn_s"] is None else "%.2f" % s["sklearn_s"]))


if __name__ == "__main__":
    main()
