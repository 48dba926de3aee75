"""Writes tests/golden/skltsne/skltsne.npz and tests/golden/skltsne.json (the arrays in a directory of their own, like the other
projection goldens: every .npz directly under tests/golden is taken for a scan case): what sklearn 1.7's own functions compute for the SKL-TSNE cases, recorded on the
CPU, and the constants of the test bounds calibrated against the long double restatements of tests/skltsne_oracle.py.

    python tools/make_skltsne_golden.py

Affinities come from _joint_probabilities / _joint_probabilities_nn (the kNN graph from NearestNeighbors, as TSNE.fit builds it);
descent states from the transcription of _gradient_descent in tests/skltsne_oracle.py driving sklearn's _kl_divergence and
_kl_divergence_bh(angle=0.0, num_threads=1); the end-to-end ensembles from TSNE(...) itself.  The GPU tests read these files only.
"""
import json
import os
import sys
import warnings

import numpy as np
from scipy.spatial.distance import squareform
from scipy.sparse import csr_matrix
from sklearn.decomposition import PCA
from sklearn.manifold import TSNE
from sklearn.manifold import _t_sne as T
from sklearn.metrics import pairwise_distances
from sklearn.neighbors import NearestNeighbors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skltsne_oracle as O      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "skltsne")
NPZ = os.path.join(OUT, "skltsne.npz")
WHOLE_N = 130                           # affinities stored whole up to this n
BIG_ROWS = (0, 1023, 1024)              # and these rows plus the last one beyond it
REC_FULL = (0, 1, 2, 11, 49, 50, 249, 250, 251, 299, 300)
REC_SHORT = (0, 1, 250, 251)
PAIRS = ((0, 1), (1, 2), (49, 50), (249, 250), (250, 251), (299, 300))
BIG_CHECK_ROWS = (0, 1, 7, 8, 255, 256, 511, 1016, 1023, 1024)

DENSE_CASES = [("dense_n%d_f44" % n, "dirichlet", 100 + n, n, 44, 1.5 if n == 2 else 2.0 if n == 3 else 20.0)
               for n in (2, 3, 64, 65, 130, 1023, 1024, 1025)]
DENSE_CASES += [("dense_n65_f1", "uniform", 201, 65, 1, 20.0), ("dense_n65_f65", "dirichlet", 265, 65, 65, 20.0),
                ("dense_n65_f2080", "dirichlet", 280, 65, 2080, 20.0), ("dense_simplex8", "simplex", 0, 8, 8, 7.0)]
SPARSE_CASES = [("sparse_n%d" % n, "dirichlet", 300 + n, n, 44, 20.0) for n in (62, 63, 130, 1025)]
SPARSE_CASES += [("sparse_n7", "dirichlet", 309, 7, 44, 1.5), ("sparse_dup65", "duplicates", 365, 65, 44, 20.0)]
GD_N = (3, 65, 1025)
GD_DIMS = {"exact": (1, 2, 3, 5), "barnes_hut": (1, 2, 3)}


def big_rows(n):
    return sorted(set(r for r in BIG_ROWS + (n - 1,) if r < n))


def knn_graph(X, perplexity):
    k = O.n_neighbors(len(X), perplexity)
    g = NearestNeighbors(algorithm="auto", n_neighbors=k, metric="euclidean").fit(X).kneighbors_graph(mode="distance")
    g.data **= 2
    g.sort_indices()
    return g, k


def dense_case(name, kind, seed, n, f, perp, out, meta, cal):
    X = O.make_X(seed, n, f, kind)
    D = pairwise_distances(X, metric="euclidean", squared=True)
    P = squareform(T._joint_probabilities(D, perp, 0))
    Dd = O.sqdist_direct(X)
    flips = int(np.sum(D.astype(np.float32) != Dd.astype(np.float32)))
    C, beta, steps = O.ld_bisect(Dd.astype(np.float32), perp, True)
    Pl = O.ld_joint_dense(C)
    dev = float(np.max(np.abs(P.astype(O.LD) - Pl) / P.max(axis=1)[:, None]) / O.EPS64)
    cal["P_dense"].append(dev)
    meta[name] = {"kind": kind, "seed": seed, "n": n, "f": f, "perplexity": perp, "flips": flips, "dev_eps64": dev,
                  "whole": n <= WHOLE_N}
    out[name + "/beta"] = beta.astype(np.float64)
    out[name + "/steps"] = steps
    out[name + "/rowsum"] = P.sum(axis=1)
    out[name + "/rowmax"] = P.max(axis=1)
    if n <= WHOLE_N:
        out[name + "/P"] = P
    else:
        out[name + "/rows"] = np.array(big_rows(n))
        out[name + "/P_rows"] = P[big_rows(n)]
    return steps


def direct_neighbours(X, k):
    """The k nearest of every row by float32-rounded direct-difference distances, ties to the lower column, columns ascending; and
    the smallest relative gap between the k-th and the (k + 1)-th float64 distance of a row."""
    n = len(X)
    Dd = O.sqdist_direct(X)
    D32 = Dd.astype(np.float32)
    idx = np.empty((n, k), dtype=np.int32)
    gap = np.inf
    for i in range(n):
        others = np.array([j for j in range(n) if j != i])
        order = others[np.lexsort((others, D32[i, others]))]
        idx[i] = np.sort(order[:k])
        if k < n - 1:
            a, b = Dd[i, order[k - 1]], Dd[i, order[k]]
            gap = min(gap, (b - a) / b if b > 0 else 0.0)
    return idx, D32, gap


def sparse_case(name, kind, seed, n, f, perp, out, meta, cal):
    X = O.make_X(seed, n, f, kind)
    g, k = knn_graph(X, perp)
    idx_sk = g.indices.reshape(n, k).astype(np.int32)
    d32 = g.data.reshape(n, k).astype(np.float32)
    cond = T._utils._binary_search_perplexity(d32, perp, 0)
    P = T._joint_probabilities_nn(g.copy(), perp, 0).tocsr()
    P.sort_indices()
    idx, D32, gap = direct_neighbours(X, k)
    assert np.array_equal(idx, idx_sk), "%s: sklearn's neighbour sets differ from the direct-difference ones" % name
    if kind != "duplicates":
        assert gap >= 1e-9, "%s: the k-th and (k+1)-th distances of a row are closer than 1e-9 (%g)" % (name, gap)
    kept32 = np.take_along_axis(D32, idx.astype(np.int64), axis=1)
    flips = int(np.sum(kept32 != d32))
    C, beta, steps = O.ld_bisect(kept32, perp, False)
    rowmax = cond.max(axis=1)
    assert np.all(C[rowmax == 0] == 0), "%s: a row sklearn leaves all zero is not zero in the restatement" % name
    dev = float(np.max(np.abs(cond.astype(O.LD) - C)[rowmax > 0] / rowmax[rowmax > 0, None]) / O.EPS64)
    cal["P_sparse"].append(dev)
    meta[name] = {"kind": kind, "seed": seed, "n": n, "f": f, "perplexity": perp, "k": k, "flips": flips, "dev_eps64": dev,
                  "min_gap": None if not np.isfinite(gap) else float(gap), "whole": n <= WHOLE_N,
                  "zero_rows": int(np.sum(rowmax == 0))}
    out[name + "/beta"] = beta.astype(np.float64)
    out[name + "/steps"] = steps
    out[name + "/joint_rowsum"] = np.asarray(P.sum(axis=1)).ravel()
    out[name + "/joint_nnz"] = np.diff(P.indptr).astype(np.int32)
    if n <= WHOLE_N:
        out[name + "/idx"] = idx_sk
        out[name + "/cond"] = cond
        out[name + "/joint_indptr"] = P.indptr.astype(np.int64)
        out[name + "/joint_indices"] = P.indices.astype(np.int32)
        out[name + "/joint_data"] = P.data
    else:
        out[name + "/rows"] = np.array(big_rows(n))
        out[name + "/idx_rows"] = idx_sk[big_rows(n)]
        out[name + "/cond_rows"] = cond[big_rows(n)]


# ---------------------------------------------------------------------------------------------------------------- descent
def affinities_of(method, X, perp):
    """(P as sklearn's objective takes it, the objective, its extra keyword arguments)."""
    if method == "exact":
        P = T._joint_probabilities(pairwise_distances(X, metric="euclidean", squared=True), perp, 0)
        return P, T._kl_divergence, {}
    g, _k = knn_graph(X, perp)
    return T._joint_probabilities_nn(g, perp, 0), T._kl_divergence_bh, {"angle": 0.0, "num_threads": 1}


def mul4(P):
    P *= 4.0
    return P


def div4(P):
    P /= 4.0
    return P


def times(method, P, ex):
    return P * ex if method == "exact" else csr_matrix((P.data * ex, P.indices, P.indptr), shape=P.shape)


def ld_objective(method, Y32, P, dof, ex):
    if method == "exact":
        return O.ld_objective_exact(Y32, squareform(P) * ex, dof)
    val32 = (P.data * ex).astype(np.float32)
    return O.ld_objective_bh(Y32, P.indptr, P.indices, val32, dof)


def one_step(method, objective, extra, P, dof, state, momentum, ex, cal):
    """sklearn's objective and one transcribed step from `state` = (Y, update, gains) float32 n x d with P x ex: the state after,
    the error, the gradient, the norm; and the deviations from the long double restatement into cal."""
    from scipy import linalg
    Y, U, G = state
    n, d = Y.shape
    err, grad = objective(Y.ravel().copy(), times(method, P, ex), dof, n, d, skip_num_points=0, compute_error=True, **extra)
    p, u, g, gg = O.gd_step(Y.ravel(), U.ravel(), G.ravel(), grad, momentum)
    err_l, grad_l, scale = ld_objective(method, Y, P, dof, ex)
    gmax = float(np.max(np.abs(grad_l)))
    cal["grad_" + method].append(float(np.max(np.abs(grad.reshape(n, d).astype(O.LD) - grad_l)) / gmax / O.EPS32))
    cal["err_" + method].append(float(abs(O.LD(err) - err_l) / scale / (O.EPS64 if method == "exact" else O.EPS32)))
    return ((p.reshape(n, d), u.reshape(n, d), g.reshape(n, d)), float(err), grad.reshape(n, d), float(linalg.norm(gg)), gmax,
            float(scale))


def gd_cases(out, meta, cal, horizon):
    for method in ("exact", "barnes_hut"):
        for n in GD_N:
            perp = 2.0 if n == 3 else 20.0
            X = O.make_X(400 + n, n, 44)
            P, objective, extra = affinities_of(method, X, perp)
            for d in GD_DIMS[method]:
                name = "gd_%s_n%d_d%d" % (method, n, d)
                dof = max(d - 1, 1)
                m = {"method": method, "seed": 400 + n, "n": n, "f": 44, "perplexity": perp, "d": d, "steps": []}
                meta[name] = m
                if n == 1025:
                    for which, momentum, ex in (("start", 0.5, 4.0), ("mid", 0.8, 1.0)):
                        st = O.synthetic_state(500 + d, n, d, which)
                        after, err, grad, norm, gmax, scale = one_step(method, objective, extra, P, dof, st, momentum, ex, cal)
                        rows = np.array(BIG_CHECK_ROWS)
                        for nm, a in zip("YUG", after):
                            out["%s/%s_after_%s" % (name, which, nm)] = a[rows]
                        out["%s/%s_grad" % (name, which)] = grad[rows]
                        m["steps"].append({"state": which, "state_seed": 500 + d, "momentum": momentum, "exaggeration": ex,
                                           "error": err, "grad_norm": norm, "gmax": gmax, "err_scale": scale,
                                           "rows": list(BIG_CHECK_ROWS)})
                    continue
                Y0 = O.random_start(600 + d, n, d)
                wanted = REC_FULL if d == 2 else REC_SHORT
                states = {}

                def record(stage, i, p, u, g):
                    if i in wanted:
                        states[i] = (stage, p.reshape(n, d).copy(), u.reshape(n, d).copy(), g.reshape(n, d).copy())
                Y, kl, n_iter, c1, c2 = O.tsne_descent(objective, Y0, P.copy(), dof, mul4, div4, extra, record)
                out[name + "/Y_final"] = Y
                m.update({"start_seed": 600 + d, "kl_divergence": float(kl), "n_iter": int(n_iter), "checks_stage1": c1,
                          "checks_stage2": c2, "recorded": sorted(states)})
                for i, (stage, p, u, g) in states.items():
                    for nm, a in zip("YUG", (p, u, g)):
                        out["%s/s%d_%s" % (name, i, nm)] = a
                for a, b in PAIRS:
                    if a in states and b in states and states[a][0] == states[b][0]:
                        momentum, ex = (0.5, 4.0) if states[a][0] == 1 else (0.8, 1.0)
                        after, err, grad, norm, gmax, scale = one_step(method, objective, extra, P, dof, states[a][1:], momentum, ex,
                                                                       cal)
                        assert all(np.array_equal(x, y) for x, y in zip(after, states[b][1:])), (name, a)
                        out["%s/s%d_grad" % (name, a)] = grad
                        m["steps"].append({"from": a, "to": b, "momentum": momentum, "exaggeration": ex, "error": err,
                                           "grad_norm": norm, "gmax": gmax, "err_scale": scale})
                if d == 2 and 11 in states and n == 65:
                    horizon.append((name, method, objective, extra, P.copy(), dof, n, d, Y0, states[11][1]))


def measure_horizon(meta, horizon):
    """The short horizon (iterations 0 .. 10 from the golden start): the trajectory amplifies a difference in the gradient, so the
    bound is measured by giving sklearn's own gradient, at every one of the 11 steps, a perturbation of the size the per-step bound
    allows (C x eps32 x max|grad|, random signs) and taking the worst relative deviation of Y over 8 draws."""
    for name, method, objective, extra, P, dof, n, d, Y0, ref in horizon:
        Cg = meta["calibration"]["grad_" + method]["C"]
        devs = []
        for draw in range(8):
            rs = np.random.RandomState(900 + draw)

            def noisy(p, *a, **kw):
                e, g = objective(p, *a, **kw)
                noise = np.float32(Cg * O.EPS32 * np.max(np.abs(g))) * rs.choice(np.array([-1, 1], np.float32), g.shape)
                return e, (g + noise).astype(np.float32)
            p, _e, _i, _u, _g, _c = O.gradient_descent(noisy, Y0.ravel(), 0, 11, 50, 250, 0.5, args=[mul4(P.copy()), dof, n, d],
                                                       kwargs=dict(extra, skip_num_points=0))
            devs.append(float(np.max(np.abs(p.reshape(n, d) - ref)) / np.max(np.abs(ref))))
        meta[name]["horizon_dev"] = max(devs)
        meta[name]["horizon_devs"] = devs


def stop_rule_and_ensembles(out, meta):
    X = O.make_X(700, 300, 44)
    seqs = {}
    for method in ("exact", "barnes_hut"):
        P, objective, extra = affinities_of(method, X, 20.0)
        _Y, kl, n_iter, c1, c2 = O.tsne_descent(objective, O.random_start(0, 300, 2), P, 1, mul4, div4, extra)
        seqs[method] = {"kl_divergence": float(kl), "n_iter": int(n_iter), "checks_stage1": c1, "checks_stage2": c2}
    ens = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for label, method, angle in (("exact", "exact", 0.5), ("barnes_hut_angle0", "barnes_hut", 0.0),
                                     ("barnes_hut_angle0.5", "barnes_hut", 0.5)):
            kls, its = [], []
            for seed in range(8):
                t = TSNE(n_components=2, perplexity=20.0, early_exaggeration=4.0, learning_rate=1000.0, max_iter=1000,
                         n_iter_without_progress=30, min_grad_norm=1e-07, metric="euclidean", init="random", random_state=seed,
                         method=method, angle=angle)
                t.fit_transform(X)
                kls.append(float(t.kl_divergence_))
                its.append(int(t.n_iter_))
            ens[label] = {"kl_divergence": kls, "n_iter": its}
    # init='pca': sklearn's randomized start against the exact PCA (sklearn's full solver stands in for projection.pca on the CPU)
    devs = []
    for seed in range(8):
        a = PCA(n_components=2, svd_solver="randomized", random_state=np.random.RandomState(seed)).fit_transform(X).astype(np.float32)
        a = a / np.std(a[:, 0]) * 1e-4
        b = PCA(n_components=2, svd_solver="full").fit_transform(X).astype(np.float32)
        b = b / np.std(b[:, 0]) * 1e-4
        devs.append(float(np.max(np.abs(a - b)) / 1e-4))
        if seed == 0:
            out["e2e/Y0_pca_sklearn"] = a
    meta["e2e"] = {"seed": 700, "n": 300, "f": 44, "perplexity": 20.0, "transcribed": seqs, "ensembles": ens,
                   "pca_start_dev": max(devs), "pca_start_devs": devs}


def main():
    out, meta = {}, {}
    cal = {k: [] for k in ("P_dense", "P_sparse", "grad_exact", "grad_barnes_hut", "err_exact", "err_barnes_hut")}
    for case in DENSE_CASES:
        steps = dense_case(*case, out, meta, cal)
        if case[0] == "dense_n2_f44":
            assert np.all(steps == 100), steps          # one neighbour: the entropy is 0 at every beta
        if case[0] == "dense_simplex8":
            assert np.all(steps == 0), steps            # seven equidistant neighbours: the entropy is log 7 at every beta
    for case in SPARSE_CASES:
        sparse_case(*case, out, meta, cal)
    horizon = []
    gd_cases(out, meta, cal, horizon)
    stop_rule_and_ensembles(out, meta)
    # every bound is C x eps x scale with C = 4 x the worst deviation of sklearn's value from the long double restatement
    meta["calibration"] = {k: {"worst": max(v), "C": 4.0 * max(v), "cases": len(v)} for k, v in cal.items()}
    measure_horizon(meta, horizon)
    meta["flips"] = {"dense": sum(m["flips"] for k, m in meta.items() if k.startswith("dense_")),
                     "sparse": sum(m["flips"] for k, m in meta.items() if k.startswith("sparse_"))}
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(NPZ, **out)
    with open(OUT + ".json", "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
    print(json.dumps(meta["calibration"], indent=1), meta["flips"], os.path.getsize(NPZ))


if __name__ == "__main__":
    main()
