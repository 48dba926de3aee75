"""MDS without a GPU: the goldens of tools/make_golden_mds.py (regenerated inputs and their hashes, the recorded runs' own
consistency), the numpy restatement of tests/mds_oracle.py against sklearn's recorded steps within its bounds, the CLI's mapping
of MDS to a built projection and the declared C ABI."""
import hashlib
import json
import os

import numpy as np
import pytest

import mds_oracle as MO
from golden_util import GOLD

G = json.load(open(os.path.join(GOLD, "mds.json")))
CASES = sorted(G["cases"])


def A(case):
    return np.load(os.path.join(GOLD, "mds", G["cases"][case]["file"]))


def make_X(spec):
    """The case's input, regenerated as tools/make_golden_mds.py make_X draws it (legacy RandomState streams are frozen)."""
    rs = np.random.RandomState(spec["seed"])
    n, dups = spec["n"], spec["dups"]
    sizes = [n // 3 + (1 if b < n % 3 else 0) for b in range(3)]
    rows = []
    for m in sizes:
        centre = [rs.dirichlet(np.full(w, 2.0)) for w in spec["orders"]]
        for _ in range(m):
            rows.append(np.concatenate([rs.dirichlet(c * spec["spread"] + 1e-3) for c in centre]))
    X = np.array(rows)[rs.permutation(n)]
    if dups:
        X[n - dups:] = X[rs.randint(0, n - dups, dups)]
    return X


def sha(X):
    return hashlib.sha256(np.ascontiguousarray(X, dtype=np.float64).tobytes()).hexdigest()


def X_of(case):
    X = make_X(G["cases"][case]["X"])
    assert sha(X) == G["cases"][case]["X"]["sha256"]
    return X


def coincident_X():
    return np.random.RandomState(77).rand(12, 5)


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", CASES)
def test_golden_inputs_regenerate_and_runs_are_consistent(case):
    g, a = G["cases"][case], A(case)
    X = X_of(case)
    assert X.shape == (g["n"], g["F"])
    assert len(g["stresses"]) == len(g["n_iters"]) == G["n_init"]
    best = int(np.argmin(g["stresses"]))
    assert best == g["best_start"] and g["stress"] == g["stresses"][best] and g["n_iter"] == g["n_iters"][best]
    rs = np.random.RandomState(g["seed"])
    for k in range(G["n_init"]):
        Y0 = rs.uniform(size=g["n"] * g["dims"]).reshape(g["n"], g["dims"])
        assert np.array_equal(Y0, a["Y0_%d" % k])
        states, st = a["states_%d" % k], a["stress_%d" % k]
        assert states.shape == (g["n_iters"][k] + 1, g["n"], g["dims"]) and st.shape == (g["n_iters"][k],)
        assert np.array_equal(states[0], Y0) and st[-1] == g["stresses"][k]
        assert g["n_iters"][k] <= g["max_iter"]
    assert g["stop_margin"] >= G["margin"] and g["best_gap"] >= G["margin"]
    assert g["mds_n_iter"] == g["n_iter"]
    # the recorded rows of D: the direct form and sklearn's Gram form, each within the oracle's bound of numpy's direct form
    rows = a["rows"]
    D = MO.direct_D(X, rows)
    assert np.all(np.abs(a["D_rows"] - D) <= MO.D_bound_exact(D, g["F"]))
    assert np.all(np.abs(a["Dsk_rows"] - D) <= MO.D_bound_exact(D, g["F"]) + MO.D_bound_gram(X, D, rows))
    Dfull = MO.direct_D(X)
    assert abs(Dfull.sum() - g["D_sum"]) <= MO.D_bound_exact(Dfull, g["F"]).sum()
    if g["dups"]:
        assert (D == 0).sum() > len(rows) or (Dfull == 0).sum() > g["n"]


def _step_ratios(X, g, a):
    """Worst ratio of |oracle step - sklearn's recorded step| to the oracle's bound, over every recorded state, and of the stress."""
    D = MO.direct_D(X)
    worst_y = worst_s = 0.0
    for k in range(G["n_init"]):
        states, st = a["states_%d" % k], a["stress_%d" % k]
        for t in range(len(st)):
            Y1 = MO.step(states[t], D)
            b = MO.step_bound(states[t], D)
            worst_y = max(worst_y, float(np.max(np.abs(Y1 - states[t + 1]) / b)))
            s1, _ = MO.stress(Y1, D)
            worst_s = max(worst_s, abs(s1 - st[t]) / MO.stress_bound(Y1, D, b))
    return worst_y, worst_s


@pytest.mark.parametrize("case", CASES)
def test_oracle_steps_match_sklearn_within_bound(case):
    g, a = G["cases"][case], A(case)
    wy, ws = _step_ratios(X_of(case), g, a)
    print("%s: worst step ratio %.3g, worst stress ratio %.3g" % (case, wy, ws))
    assert wy <= 1.0 and ws <= 1.0


def test_oracle_coincident_points_step():
    c = G["coincident"]
    a = np.load(os.path.join(GOLD, "mds", c["file"]))
    X = coincident_X()
    assert sha(X) == c["X"]["sha256"]
    D = MO.direct_D(X)
    assert np.array_equal(D, a["D"])
    Y = a["Y"]
    assert np.array_equal(Y[0], Y[1]) and D[0, 1] > 0
    Y1 = MO.step(Y, D)
    assert np.all(np.abs(Y1 - a["Y1"]) <= MO.step_bound(Y, D))
    assert abs(MO.stress(Y1, D)[0] - c["stress1"]) <= MO.stress_bound(Y1, D, MO.step_bound(Y, D))


def test_full_runs_of_the_oracle_reach_the_recorded_result():
    """the oracle iterated with sklearn's stop rule reproduces n_iter of every start, for two cases"""
    for case in ("blobs44", "d3"):
        g, a = G["cases"][case], A(case)
        D = MO.direct_D(X_of(case))
        for k in range(G["n_init"]):
            Y, old = a["Y0_%d" % k], None
            for it in range(g["max_iter"]):
                Y = MO.step(Y, D)
                s, ss = MO.stress(Y, D)
                if old is not None and (old - s) / ss < g["eps"]:
                    break
                old = s
            assert it + 1 == g["n_iters"][k]
            assert np.max(np.abs(Y - a["states_%d" % k][-1])) <= 1e-9 * np.max(np.abs(Y))


# ------------------------------------------------------------------------------------------------ CLI and ABI
def test_cli_maps_mds_to_a_built_projection():
    from frisk_amd import postprocess as pp
    from frisk_amd.cli import PROJECTIONS, build_parser, unavailable
    assert "MDS" in PROJECTIONS
    for clust in ("DBSCAN", "KMEANS"):
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "MDS", "--cluster", clust])
        assert unavailable(args) == []
    args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "MDS", "--cluster", "SPECTRAL"])
    assert ("cluster", "sklearn clustering is out of scope") in unavailable(args)
    e = G["e2e"]
    args = build_parser().parse_args(e["argv"] + ["-H", "x.fa"])
    assert pp.clusterGffName(args) == e["cluster_gff_name"]
    args = build_parser().parse_args(e["argv"][:-6] + ["--cluster", "KMEANS", "-H", "x.fa", "--gffOutfile", "a.gff3"])
    assert pp.clusterGffName(args) == e["kmeans_gff_name"]


def test_mds_constants_follow_the_reference():
    from frisk_amd import projection as P
    assert (P.MDS_N_INIT, P.MDS_MAX_ITER, P.MDS_EPS, P.MDS_MAX_N) == (5, 500, 1e-3, 50000)


def test_mds_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    want = {"frisk_mds_create", "frisk_mds_dissimilarities", "frisk_mds_run", "frisk_mds_destroy"}
    assert want <= names
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "frisk_hip.h")).read()
    for name in want:
        assert name + "(" in header
