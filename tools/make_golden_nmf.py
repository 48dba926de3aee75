#!/usr/bin/env python3
"""Goldens of the NMF projection (sklearn.decomposition.NMF(n_components=d, init=None, solver='cd', tol=0.0001, max_iter=200,
shuffle=False), called at frisk/__init__.py L1632-1636 as .fit(X).transform(X)): tests/golden/nmf.json and one compressed .npz per
case under tests/golden/nmf/.  sklearn 1.7; the reference passes random_state=None, the goldens a seed.

Inputs are Dirichlet-multinomial rows (tests/nmf_oracle.make_X): non-negative and proportion-like, stored in the .npz with their
generator call and sha256.  Per case:
  * sklearn's _randomized_svd(X, d, random_state=seed) (U, S, V) where d <= min(n, f), and _initialize_nmf's (W0, H0);
  * the fit step by step: chained _update_coordinate_descent calls (what _fit_coordinate_descent runs), with the stop rule applied
    here, asserted bit-equal to NMF.fit's components_ and n_iter_; recorded are (W_t, H_t), (W_t+1, H_t+1) and the violation of
    the step between them for every t, thinned to every 10th and the last three where the fit is longer than 30 iterations;
  * every violation ratio; the same for the transform (W from zeros, H fixed), asserted bit-equal to NMF.transform;
  * run_gap: the largest |difference| in Y and in components_ between sklearn's run and the run of tests/nmf_oracle.py with
    pairwise-order sums (start included): two honest double implementations, the yardstick of the GPU's full-run test.
Asserted per case (the seed is advanced until sklearn alone meets them):
  * no entry of the NNDSVD split before its cut lies within 1e-9 of 1e-6;
  * at the stopping iteration and the one before it, violation / violation_init is at least 1e-3 relative away from tol, in the
    fit and in the transform, under sklearn and under the pairwise run, which must stop at the same iterations;
  * m_p and m_n of every NNDSVD column differ by more than 1e-9 relative.
This script does not use the package under test.

    python tools/make_golden_nmf.py

A second table, tests/golden/nmf_edges.json with tests/golden/nmf_edges/*.npz (EDGE_CASES: d at the inner edges of the sweep
kernel's copies, absent k-mers and an empty row, duplicated rows, rank 1, n = 1, f = 1), is written by

    python tools/make_golden_nmf.py --edges

and leaves the first untouched.  Its rules are the same, with two differences.  Recorded states are thinned to the first, the
middle and the last three.  Where X has rank below d the null triplets (singular value below 1e-12 of the first) are directions
of rounding noise, different in every implementation, and m_p against m_n means nothing for them: instead of the split margin,
everything they put into the split must lie below the 1e-6 cut by the cut margin, so that every implementation starts those
components from the mean of X.  A case that sklearn alone cannot bring within the margins in 50 seeds is left out and named.
"""
import hashlib
import json
import os
import sys
import warnings

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"            # one BLAS thread: one summation order, the same last bits every run
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import nmf_oracle as NO  # noqa: E402

GOLD = NO.GOLD
ARR = os.path.join(GOLD, "nmf")
TOL, MAX_ITER = 1e-4, 200
CUT_MARGIN, STOP_MARGIN, SPLIT_MARGIN = 1e-9, 1e-3, 1e-9
THIN_ABOVE = 30

# name: (n, orders (f = their sum), d, first seed, what it exercises)
CASES = {
    "base": (44, (10,), 2, 1, "baseline"),
    "odd": (67, (4, 32), 3, 2, "f and n off every tile multiple"),
    "wide": (130, (3, 32, 100), 2, 3, "n < f: the transposed range finder; 4 power iterations"),
    "tiny": (9, (5,), 2, 4, "smaller than one tile; the range finder narrower than d + 10"),
    "n257": (257, (4, 32), 5, 5, "one row past a 256 tile; sklearn reaches max_iter"),
    "random": (3, (10,), 4, 6, "d > min(n, f): the 'random' start"),
    "d16": (20, (44, 256), 16, 7, "d at its cap, p = 26"),
    "d1": (30, (2, 10), 1, 8, "d = 1: only the leading triplet"),
}
# name: (n, orders, d, first seed, what it exercises, further fields of the input spec (tests/nmf_oracle.make_X))
EDGE_CASES = {
    "d8": (100, (4, 64), 8, 1, "nmf_sweep<8> at its upper edge", {}),
    "d9": (60, (36, 100), 9, 2, "nmf_sweep<16> at its lower edge; n < f: the transposed range finder", {}),
    "absent": (260, (8, 32), 4, 3, "three all-zero columns and one all-zero row", {"absent": {"cols": [0, 17, 39], "rows": [101]}}),
    "dups": (90, (4, 16), 5, 4, "rows drawn from three distinct rows: rank 3 below d = 5", {"distinct": 3}),
    "rank1": (50, (12,), 3, 5, "an outer product: two null triplets", {"rank1": True}),
    "n1d1": (1, (10,), 1, 6, "one row, d = 1", {}),
    "n1d3": (1, (10,), 3, 7, "one row, d = 3: the 'random' start", {}),
    "f1": (40, (1,), 1, 8, "one feature, d = 1", {}),
}
NULL_TRIPLET = 1e-12
EDGE_SEEDS = 50


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def chain(X, W, H, update_H):
    """(states [(W_0, H_0), ...], violations of every step, ratios, n_iter) of _fit_coordinate_descent run step by step."""
    from sklearn.decomposition._nmf import _update_coordinate_descent
    from sklearn.utils import check_array
    W = W.copy()
    Ht = check_array(H.T, order="C")
    states, viols, ratios = [(W.copy(), Ht.T.copy())], [], []
    init = None
    for it in range(1, MAX_ITER + 1):
        v = 0.0
        v += _update_coordinate_descent(X, W, Ht, 0, 0, False, None)
        if update_H:
            v += _update_coordinate_descent(X.T, Ht, W, 0, 0, False, None)
        states.append((W.copy(), Ht.T.copy()))
        viols.append(float(v))
        if it == 1:
            init = v
        if init == 0:
            break
        ratios.append(float(v / init))
        if v / init <= TOL:
            break
    return states, viols, ratios, it


def margins_ok(ratios, n_iter):
    return all(abs(r - TOL) / TOL >= STOP_MARGIN for r in ratios[-2:])


def thin(T, edges=False):
    if edges:
        return sorted({0, T // 2} | set(range(max(0, T - 3), T)))
    return [t for t in range(T) if T <= THIN_ABOVE or t % 10 == 0 or t >= T - 3]


def one(name, n, orders, d, seed, extra=None, edges=False):
    from sklearn.decomposition import NMF
    from sklearn.decomposition._nmf import _initialize_nmf
    from sklearn.utils.extmath import _randomized_svd
    spec = dict({"seed": 1000 + seed, "n": n, "orders": list(orders), "spread": 40.0, "depth": 400}, **(extra or {}))
    X = NO.make_X(spec)
    f = X.shape[1]
    arr = {"X": X}
    doc = {"n": n, "f": f, "d": d, "seed": seed, "X": dict(spec, sha256=sha(X)), "init": "nndsvda" if d <= min(n, f) else "random"}
    if d <= min(n, f):
        U, S, V = _randomized_svd(X, d, random_state=seed)
        arr.update(U=U, S=S, V=V)
        Wr, Hr, ms = NO.nndsvd_raw(U, S, V)
        if min(np.abs(Wr - 1e-6).min(), np.abs(Hr - 1e-6).min()) <= CUT_MARGIN:
            return None
        null = [j for j in range(1, d) if edges and S[j] < NULL_TRIPLET * S[0]]
        if any(max(Wr[:, j].max(), Hr[j].max()) >= 1e-6 - CUT_MARGIN for j in null):
            return None
        ms = [m for j, m in enumerate(ms, 1) if j not in null]
        if any(abs(a - b) <= SPLIT_MARGIN * max(a, b) for a, b in ms):
            return None
        if edges:
            doc["null_triplets"] = null
        doc["split_margin"] = min([abs(a - b) / max(a, b) for a, b in ms] or [1.0])
        doc["cut_margin"] = float(min(np.abs(Wr - 1e-6).min(), np.abs(Hr - 1e-6).min()))
    W0, H0 = _initialize_nmf(X, d, init=None, random_state=seed)
    arr.update(W0=W0.copy(), H0=np.ascontiguousarray(H0).copy())
    states, viols, ratios, n_iter = chain(X, W0, H0.copy(), True)       # (check_array(H.T) may alias H: H0 is F-ordered)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = NMF(n_components=d, init=None, solver="cd", tol=TOL, max_iter=MAX_ITER, random_state=seed, shuffle=False).fit(X)
        Y = model.transform(X)
    assert model.n_iter_ == n_iter and np.array_equal(model.components_, states[-1][1]), (name, model.n_iter_, n_iter)
    H = model.components_
    tstates, tviols, tratios, t_iter = chain(X, np.zeros((n, d)), H, False)
    assert np.array_equal(Y, tstates[-1][0]), name
    if not (margins_ok(ratios, n_iter) and margins_ok(tratios, t_iter)):
        return None
    if name == "n257" and not (n_iter == MAX_ITER and ratios[-1] > TOL):        # this case is the one that must not converge
        return None
    # the pairwise run: the second double implementation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pw = NO.fit_transform(X, d, seed, TOL, MAX_ITER, how="pairwise")
    if (pw["n_iter"], pw["transform_n_iter"]) != (n_iter, t_iter):
        return None
    doc["run_gap"] = {"Y": float(np.abs(pw["Y"] - Y).max()), "components": float(np.abs(pw["components"] - H).max())}
    ts = thin(n_iter, edges)
    arr.update(fit_t=np.array(ts), fit_W=np.array([states[t][0] for t in ts]), fit_H=np.array([states[t][1] for t in ts]),
               fit_W1=np.array([states[t + 1][0] for t in ts]), fit_H1=np.array([states[t + 1][1] for t in ts]),
               fit_v=np.array([viols[t] for t in ts]), ratios=np.array(ratios), components=H, Y=Y)
    tt = thin(t_iter, edges)
    arr.update(tr_t=np.array(tt), tr_W=np.array([tstates[t][0] for t in tt]), tr_W1=np.array([tstates[t + 1][0] for t in tt]),
               tr_v=np.array([tviols[t] for t in tt]), tr_ratios=np.array(tratios))
    doc.update(n_iter=n_iter, transform_n_iter=t_iter, hit_max_iter=bool(n_iter == MAX_ITER and ratios[-1] > TOL),
               last_ratio=ratios[-1] if ratios else 0.0, zeros_in_Y=int((Y == 0).sum()), max_abs_Y=float(np.abs(Y).max()),
               file=name + ".npz")
    return doc, arr


def main(edges=False):
    import sklearn
    assert sklearn.__version__.startswith("1.7"), sklearn.__version__
    table = "nmf_edges" if edges else "nmf"
    arr_dir = os.path.join(GOLD, table)
    os.makedirs(arr_dir, exist_ok=True)
    out = {"sklearn": sklearn.__version__, "tol": TOL, "max_iter": MAX_ITER, "cases": {}}
    if edges:
        out.update(dir=table, left_out=[])
    for name, case in (EDGE_CASES if edges else CASES).items():
        n, orders, d, seed, what = case[:5]
        for s in range(seed, seed + 8 * (EDGE_SEEDS if edges else 50), 8):      # the case's own residue class of seeds
            got = one(name, n, orders, d, s, *((case[5], True) if edges else ()))
            if got is not None:
                break
        else:
            if not edges:
                raise SystemExit("no seed of case %s meets the conditions" % name)
            out["left_out"].append(name)
            print("%-7s left out: no seed of %d meets the conditions" % (name, EDGE_SEEDS))
            continue
        doc, arr = got
        doc["exercises"] = what
        np.savez_compressed(os.path.join(arr_dir, doc["file"]), **arr)
        out["cases"][name] = doc
        print("%-7s n=%d f=%d d=%d seed=%d n_iter=%d transform=%d run_gap=%s" % (name, n, doc["f"], d, doc["seed"], doc["n_iter"],
                                                                               doc["transform_n_iter"], doc["run_gap"]))
    with open(os.path.join(GOLD, table + ".json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(edges="--edges" in sys.argv[1:])
