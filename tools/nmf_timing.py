#!/usr/bin/env python3
"""Device time of the NMF kernels (csrc/nmf_kernels.h) and wall-clock of projection.nmf at the size of a large anomaly set:
n = 20 000 windows x f = 2 772 k-mer proportions (orders 1..6), d = 2.  X Q and XT Q' (p = d and p = d + 10, the range finder's
width) and one coordinate-descent step are timed with the handle's HIP events: one warm-up, then the median of --repeats calls.
Each product reads X once, 8 n f bytes, so bytes / time is set against the HBM rate (--hbm-gbs, 8000 for an MI355X) as the
achieved fraction.  The whole fit and transform are wall-clock, once after a warm-up.  With --sklearn the same case runs through
sklearn's NMF on the host's CPU (not part of the package; the only comparison there is).  Prints one JSON line and a markdown
table.  Runs no test.

    python tools/nmf_timing.py [--n 20000] [--dims 2] [--repeats 11] [--sklearn] [--device 0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

ORDERS = (2, 10, 32, 136, 512, 2080)        # kept words of orders 1..6: f = 2 772


def kmer_like(n, seed=41, blobs=4):
    """Rows of per-order proportions around `blobs` Dirichlet centres."""
    rs = np.random.RandomState(seed)
    centres = [[rs.dirichlet(np.full(w, 2.0)) for w in ORDERS] for _ in range(blobs)]
    which = rs.randint(0, blobs, n)
    out = np.empty((n, sum(ORDERS)))
    col = 0
    for k, w in enumerate(ORDERS):
        for b in range(blobs):
            rows = np.nonzero(which == b)[0]
            out[rows, col:col + w] = rs.dirichlet(centres[b][k] * 200.0 + 1e-3, size=len(rows))
        col += w
    return out


def median_ms(call, read, repeats):
    call()
    ts = []
    for _ in range(repeats):
        call()
        ts.append(read())
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from frisk_amd import projection as P
    X = kmer_like(a.n)
    n, f = X.shape
    d = a.dims
    rs = np.random.RandomState(5)
    res = {"n": n, "f": f, "d": d, "x_bytes": 8 * n * f}
    with P.NMF(X, d, a.device) as h:
        for p in (d, d + P.NMF_OVERSAMPLES):
            Qf, Qn = rs.normal(size=(f, p)), rs.normal(size=(n, p))
            res["xq_p%d_ms" % p] = median_ms(lambda: h.xq(Qf), lambda: h.last_ms()[0], a.repeats)
            res["xtq_p%d_ms" % p] = median_ms(lambda: h.xtq(Qn), lambda: h.last_ms()[1], a.repeats)
        W0, H0 = P.nmf_init(h, X, d, 0)
        step = []
        for which in range(3):
            h.set(W0, H0)
            step.append(median_ms(lambda: h.step(True), lambda w=which: h.last_ms()[w], a.repeats))
        res["step_xht_ms"], res["step_xtw_ms"], res["step_ms"] = step
        h.set(W0, H0)
        h.transform_prepare()
        res["transform_step_ms"] = median_ms(lambda: h.step(False), lambda: h.last_ms()[2], a.repeats)
    for key in ("xq_p%d_ms" % d, "xtq_p%d_ms" % d, "xq_p%d_ms" % (d + 10), "xtq_p%d_ms" % (d + 10), "step_xht_ms", "step_xtw_ms"):
        res[key.replace("_ms", "_hbm_fraction")] = res["x_bytes"] / (res[key] * 1e-3) / (a.hbm_gbs * 1e9)
    P.nmf(X[:256], d, device=a.device)                      # warm-up of the whole path
    t0 = time.perf_counter()
    r = P.nmf(X, d, device=a.device)
    res.update(wall_s=time.perf_counter() - t0, n_iter=r.n_iter, transform_n_iter=r.transform_n_iter,
               **{k: v for k, v in r.timings.items()})
    if a.sklearn:
        import warnings
        from sklearn.decomposition import NMF
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            m = NMF(n_components=d, init=None, solver="cd", tol=1e-4, max_iter=200, random_state=0, shuffle=False).fit(X)
            t1 = time.perf_counter()
            Y = m.transform(X)
            t2 = time.perf_counter()
        res.update(sklearn_fit_s=t1 - t0, sklearn_transform_s=t2 - t1, sklearn_n_iter=int(m.n_iter_),
                   sklearn_cpus=len(os.sched_getaffinity(0)), gap_Y=float(np.abs(Y - r.Y).max()),
                   gap_components=float(np.abs(m.components_ - r.components).max()))
    print(json.dumps(res), flush=True)
    print("| what | ms | of the HBM rate |")
    print("|---|---|---|")
    for key, label in (("xq_p%d" % d, "X Q, p = %d" % d), ("xtq_p%d" % d, "XT Q', p = %d" % d),
                       ("xq_p%d" % (d + 10), "X Q, p = %d" % (d + 10)), ("xtq_p%d" % (d + 10), "XT Q', p = %d" % (d + 10)),
                       ("step_xht", "X HT within a step"), ("step_xtw", "XT W within a step")):
        print("| %s | %.3f | %.2f |" % (label, res[key + "_ms"], res[key + "_hbm_fraction"]))
    print("| one step (both sweeps) | %.3f | |" % res["step_ms"])
    print("| one transform step (products frozen) | %.3f | |" % res["transform_step_ms"])
    print("| start / fit (%d iterations) / transform (%d) | %.0f / %.0f / %.0f | |" % (
        r.n_iter, r.transform_n_iter, res["init_ms"], res["fit_ms"], res["transform_ms"]))


if __name__ == "__main__":
    main()
