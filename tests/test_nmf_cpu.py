"""NMF without a GPU: the goldens of tools/make_golden_nmf.py (inputs regenerate, the recorded margins), the numpy restatement of
tests/nmf_oracle.py against sklearn's recorded start, steps and runs, a long-double step against the oracle's derived bound, the
package's own start and stop rule driven through a numpy stand-in for the device handle, the CLI wiring and the declared C ABI."""
import hashlib
import os
import pickle

import numpy as np
import pytest

import nmf_oracle as NO

G = NO.golden()
CASES = sorted(G["cases"])
SHAPES = {(44, 10, 2), (67, 36, 3), (130, 135, 2), (9, 5, 2), (257, 36, 5), (3, 10, 4), (20, 300, 16)}


def run_tol(g, what, ref):
    """The full-run yardstick: 16 x max(run_gap, 1e-13 max|ref|), run_gap measured on the CPU between sklearn and the oracle's
    pairwise-order run (tools/make_golden_nmf.py)."""
    return 16 * max(g["run_gap"][what], 1e-13 * float(np.abs(ref).max()))


class NumpyHandle:
    """frisk_amd.projection.NMF's interface with numpy products and the oracle's step: the package's Python, no device."""

    def __init__(self, X, d):
        from frisk_amd.projection import NMF
        self.X, (self.n, self.f), self.dims = X, X.shape, d
        self.W, self.H = np.zeros((self.n, d)), np.zeros((d, self.f))
        self.iterate = lambda *a, **k: NMF.iterate(self, *a, **k)

    def xq(self, Q):
        assert Q.shape[0] == self.f and 1 <= Q.shape[1] <= 26
        return self.X @ Q

    def xtq(self, Q):
        assert Q.shape[0] == self.n and 1 <= Q.shape[1] <= 26
        return self.X.T @ Q

    def set(self, W=None, H=None):
        self.W = self.W if W is None else W.copy()
        self.H = self.H if H is None else H.copy()

    def get(self):
        return self.W.copy(), self.H.copy()

    def step(self, update_H=True):
        self.W, self.H, v = NO.step(self.X, self.W, self.H, update_H)
        return float(v)


# ------------------------------------------------------------------------------------------------ goldens
def test_goldens_cover_the_shapes_and_record_their_margins():
    assert G["sklearn"].startswith("1.7") and (G["tol"], G["max_iter"]) == (1e-4, 200)
    shapes = {(g["n"], g["f"], g["d"]) for g in G["cases"].values()}
    assert SHAPES <= shapes and any(d == 1 for _, _, d in shapes)
    assert G["cases"]["n257"]["hit_max_iter"] and G["cases"]["n257"]["n_iter"] == 200
    assert G["cases"]["random"]["init"] == "random" and G["cases"]["wide"]["n"] < G["cases"]["wide"]["f"]
    for case in CASES:
        g, a = G["cases"][case], NO.arrays(G, case)
        X = NO.make_X(g["X"])
        assert X.shape == (g["n"], g["f"]) and np.array_equal(X, a["X"])
        assert hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest() == g["X"]["sha256"]
        assert X.min() >= 0
        for ratios in (a["ratios"], a["tr_ratios"]):
            assert all(abs(r - G["tol"]) / G["tol"] >= 1e-3 for r in ratios[-2:])
        assert len(a["ratios"]) == g["n_iter"] and len(a["tr_ratios"]) == g["transform_n_iter"]
        assert (a["ratios"][-1] <= G["tol"]) != g["hit_max_iter"]
        if g["init"] == "nndsvda":
            assert g["cut_margin"] > 1e-9 and g["split_margin"] > 1e-9
        assert a["fit_t"][-1] == g["n_iter"] - 1 and np.array_equal(a["fit_H1"][-1], a["components"])
        assert a["tr_t"][-1] == g["transform_n_iter"] - 1 and np.array_equal(a["tr_W1"][-1], a["Y"])
        assert not np.any(a["tr_W"][0]) and np.array_equal(a["fit_W"][0], a["W0"]) and np.array_equal(a["fit_H"][0], a["H0"])


# ------------------------------------------------------------------------------------------------ the oracle against sklearn
@pytest.mark.parametrize("case", CASES)
def test_oracle_start_matches_sklearn(case):
    g, a = G["cases"][case], NO.arrays(G, case)
    X = a["X"]
    if g["init"] == "nndsvda":
        U, S, V = NO.randomized_svd(X, g["d"], g["seed"])
        for got, want in ((U, a["U"]), (S, a["S"]), (V, a["V"])):
            assert np.array_equal(got, want) or np.abs(got - want).max() <= 1e-14
    W0, H0 = NO.initialize(X, g["d"], g["seed"])
    assert np.array_equal(W0 == X.mean(), a["W0"] == X.mean()) and np.array_equal(H0 == X.mean(), a["H0"] == X.mean())
    assert np.abs(W0 - a["W0"]).max() <= 1e-14 and np.abs(H0 - a["H0"]).max() <= 1e-14


@pytest.mark.parametrize("case", CASES)
def test_oracle_steps_match_sklearn_within_bound(case):
    g, a = G["cases"][case], NO.arrays(G, case)
    X = a["X"]
    worst = 0.0
    for k in range(len(a["fit_t"])):
        W1, H1, v = NO.step(X, a["fit_W"][k], a["fit_H"][k])
        bW, bH, bv = NO.step_bound(X, a["fit_W"][k], a["fit_H"][k])
        for got, want, b in ((W1, a["fit_W1"][k], bW), (H1, a["fit_H1"][k], bH)):
            err = np.abs(got - want)
            assert np.all((err <= b))
            worst = max(worst, float(np.max(err[b > 0] / b[b > 0], initial=0.0)))
        assert abs(v - a["fit_v"][k]) <= bv
        worst = max(worst, abs(v - a["fit_v"][k]) / bv)
    for k in range(len(a["tr_t"])):
        W1, _H, v = NO.step(X, a["tr_W"][k], a["components"], update_H=False)
        bW, _bH, bv = NO.step_bound(X, a["tr_W"][k], a["components"], update_H=False)
        assert np.all(np.abs(W1 - a["tr_W1"][k]) <= bW) and abs(v - a["tr_v"][k]) <= bv
    print("%s: worst oracle step ratio %.3g" % (case, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_long_double_step_bounds_the_double_one(case):
    """one implementation against (nearly) exact arithmetic: sides = 1, for both double summation orders"""
    g, a = G["cases"][case], NO.arrays(G, case)
    X = a["X"]
    worst = 0.0
    for k in sorted({0, len(a["fit_t"]) // 2, len(a["fit_t"]) - 1}):
        W, H = a["fit_W"][k], a["fit_H"][k]
        Wl, Hl, vl = NO.step(X, W, H, how="ld")
        bW, bH, bv = NO.step_bound(X, W, H, sides=1)
        for how in ("blas", "pairwise"):
            W1, H1, v = NO.step(X, W, H, how=how)
            eW, eH = np.abs(W1 - Wl).astype(np.float64), np.abs(H1 - Hl).astype(np.float64)
            assert np.all(eW <= bW) and np.all(eH <= bH) and abs(float(v - vl)) <= bv
            worst = max(worst, float(np.max(eW[bW > 0] / bW[bW > 0], initial=0.0)), float(np.max(eH[bH > 0] / bH[bH > 0], initial=0.0)),
                        abs(float(v - vl)) / bv)
    print("%s: worst double / long double ratio %.3g" % (case, worst))
    assert 0 < worst <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_oracle_full_run_matches_sklearn(case):
    g, a = G["cases"][case], NO.arrays(G, case)
    r = NO.fit_transform(a["X"], g["d"], g["seed"])
    assert (r["n_iter"], r["transform_n_iter"]) == (g["n_iter"], g["transform_n_iter"])
    assert np.abs(r["components"] - a["components"]).max() <= run_tol(g, "components", a["components"])
    assert np.abs(r["Y"] - a["Y"]).max() <= run_tol(g, "Y", a["Y"])
    assert np.abs(np.array(r["ratios"]) - a["ratios"]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ the package's Python
@pytest.mark.parametrize("case", CASES)
def test_package_start_and_stop_rule_on_a_numpy_handle(case):
    """projection.nmf_init and NMF.iterate (the code that runs around the device) reproduce sklearn's start and iteration
    counts when the products and the step are numpy's"""
    from frisk_amd import projection as P
    g, a = G["cases"][case], NO.arrays(G, case)
    X = a["X"]
    h = NumpyHandle(X, g["d"])
    W0, H0 = P.nmf_init(h, X, g["d"], g["seed"])
    assert np.abs(W0 - a["W0"]).max() <= 1e-14 and np.abs(H0 - a["H0"]).max() <= 1e-14
    h.set(W0, H0)
    n_iter, ratios = h.iterate(True)
    assert n_iter == g["n_iter"] and len(ratios) == n_iter
    h.set(W=np.zeros((g["n"], g["d"])))
    t_iter, _ = h.iterate(False)
    assert t_iter == g["transform_n_iter"]
    assert np.abs(h.get()[0] - a["Y"]).max() <= run_tol(g, "Y", a["Y"])


def test_nmf_constants_and_argument_checks():
    from frisk_amd import projection as P
    assert (P.NMF_TOL, P.NMF_MAX_ITER, P.NMF_MAX_DIMS, P.NMF_MAX_P) == (1e-4, 200, 16, 26)
    X = np.random.RandomState(0).rand(6, 4)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            P.nmf(X, bad)
    with pytest.raises(ValueError, match="Negative values"):
        P.nmf(-X, 2)
    with pytest.raises(ValueError):
        P.nmf(np.full((3, 3), np.nan), 2)


# ------------------------------------------------------------------------------------------------ CLI and ABI
class Clock:
    def __init__(self):
        self.laps = []

    def lap(self, name):
        self.laps.append(name)


def _fake_nmf(calls):
    from frisk_amd.projection import NMFResult

    def nmf(X, dims, seed=0, device=0, **kw):
        calls.append((X.shape, dims, seed, device))
        Y = np.arange(X.shape[0] * dims, dtype=np.float64).reshape(X.shape[0], dims)
        return NMFResult(Y, np.ones((dims, X.shape[1])), 7, 3, [1.0, 0.5], None, None,
                         {"init_ms": 1.0, "fit_ms": 2.0, "transform_ms": 3.0})
    return nmf


@pytest.mark.parametrize("dump", [False, True])
def test_cli_dispatches_nmf_and_dumps_the_projection(tmp_path, monkeypatch, dump):
    from frisk_amd import cli, projection as P
    calls = []
    monkeypatch.setattr(P, "nmf", _fake_nmf(calls))
    argv = ["-H", "x.fa", "-t", str(tmp_path), "--runProjection", "NMF", "--projectionDims", "3", "--seed", "5",
            "--cluster", "DBSCAN"] + (["--dumpPCAdata"] if dump else [])
    args = cli.build_parser().parse_args(argv)
    clock = Clock()
    counts = np.random.RandomState(1).rand(11, 44)
    assert cli._project(args, counts, 0, clock) is None             # no labels: clustering NMF is not offered
    assert calls == [((11, 44), 3, 5, 0)] and clock.laps == ["NMF"]
    path = tmp_path / "anomNMF"
    assert path.exists() == dump
    if dump:
        Y = pickle.load(open(path, "rb"))
        assert Y.shape == (11, 3) and Y[10, 2] == 32.0
    assert os.listdir(tmp_path) == (["anomNMF"] if dump else [])


def test_cli_builds_nmf_but_not_its_clustering():
    from frisk_amd.cli import PROJECTIONS, PROJECTIONS_UNCLUSTERED, build_parser, unavailable
    assert PROJECTIONS_UNCLUSTERED == ("NMF",) and "NMF" not in PROJECTIONS
    args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "NMF"])
    assert unavailable(args) == []
    for clust in ("DBSCAN", "KMEANS", "SPECTRAL"):
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "NMF", "--cluster", clust])
        assert unavailable(args) == [("cluster", "sklearn clustering is out of scope")]


def test_nmf_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    want = {"frisk_nmf_create", "frisk_nmf_xq", "frisk_nmf_xtq", "frisk_nmf_step", "frisk_nmf_get", "frisk_nmf_set",
            "frisk_nmf_transform_prepare", "frisk_nmf_last_ms", "frisk_nmf_destroy"}
    assert want <= names
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "frisk_hip.h")).read()
    for name in want:
        assert name + "(" in header
    src = open(os.path.join(os.path.dirname(__file__), "..", "frisk_amd", "csrc", "nmf_kernels.h")).read()
    assert "NMF_MAX_P = 26" in src
