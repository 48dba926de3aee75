"""Spectral clustering without a GPU: the numpy restatement (tests/spectral_oracle.py) against sklearn's goldens (tests/golden/
spectral.json, tools/make_golden_spectral.py) - labels as a partition, the embedding's pairwise row distances and the Davis-Kahan
subspace bound; the package's own host code (projection.spectral_embedding, the rs hand-over to kmeans, the argument checks, the
CLI dispatch) on a numpy handle; the declared ABI; and the calibration of C_EXP (tests/spectral_oracle_hp.py)."""
import logging
import os
import pickle

import numpy as np
import pytest

import spectral_oracle as SO
import spectral_oracle_hp as HP

G = SO.golden()
CASES = sorted(G["cases"])
EPS = SO.EPS


host_matrix, check_embedding = SO.host_matrix, SO.check_embedding


# ------------------------------------------------------------------------------------------------ the oracle against sklearn
@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_sklearn(case):
    g = G["cases"][case]
    Y = SO.array(case, "Y")
    out = SO.pipeline(Y, g["k"], g["seed"], g["gamma"])
    dd_g = SO.array(case, "dd")
    assert out["n_isolated"] == g["n_isolated"]
    # sklearn forms |x|^2 - 2 x.y + |y|^2: it cancels where the oracle's direct differences do not, an error of a few eps64
    # (|x|^2 + |y|^2) on the exponent, so a relative one on the affinity, and at most that on the column sums
    sq = (Y * Y).sum(axis=1)
    rel = 8 * (Y.shape[1] + 2) * EPS * g["gamma"] * (sq[:, None] + sq[None, :] + 1.0)
    assert np.all(np.abs(out["dd"] - dd_g) <= (4 * g["n"] * EPS + 0.5 * rel.max()) * dd_g)
    if "affinity" in g["arrays"]:
        Ag = SO.array(case, "affinity")
        assert np.all(np.diagonal(Ag) == 1.0) and np.all(np.diagonal(out["A"]) == 0.0)        # sklearn's diagonal is exp(0)
        tol = rel * Ag + HP.DBL_MIN
        off = ~np.eye(g["n"], dtype=bool)
        assert np.all(np.abs(out["A"] - Ag)[off] <= tol[off])
    assert np.array_equal(out["M"], out["M"].T)
    assert out["residuals"].max() <= SO.TOL and out["n_iter"] < SO.MAX_ITER
    _A, dd, M = host_matrix(case)
    check_embedding(case, out["embedding"], out["eigenvalues"], out["residuals"], M, dd)
    assert SO.same_partition(out["labels"], SO.array(case, "labels")), case


def test_goldens_meet_their_own_conditions():
    assert G["min_gap"] == 0.1 and len(CASES) >= 16
    for case in CASES:
        g = G["cases"][case]
        assert g["gap_k"] >= G["min_gap"] and 2 <= g["n"] <= 700 and 1 <= g["k"] <= 16 and g["k"] < g["n"]
        assert len(set(SO.array(case, "labels").tolist())) == g["k"]
    assert G["cases"]["isolated"]["n_isolated"] == 1 and G["cases"]["minus_one"]["lambda_min"] < -0.999
    assert G["cases"]["p_eq_n"]["n"] <= G["cases"]["p_eq_n"]["k"] + SO.GUARD
    assert {G["cases"][c]["n"] for c in CASES} >= {2, 63, 64, 65, 255, 256, 257, 517, 645}


def test_mirror_mean_is_within_one_ulp_of_scipy():
    """why the device writes (r + r') / 2: scipy's entry and its mirror differ by up to 2 ulps, their mean by at most 1 from either"""
    A, dd, M = host_matrix("n645")
    S = SO.scipy_matrix(A, dd)
    ulp = np.spacing(np.minimum(S, S.T))
    assert np.abs(S - S.T).max() > 0 and np.all(np.abs(S - S.T) <= 2 * ulp)
    assert np.all(np.abs(M - S) <= ulp) and np.all(np.abs(M - S.T) <= ulp) and np.array_equal(M, M.T)


# ------------------------------------------------------------------------------------------------ the package's Python
class NumpyHandle:
    """What projection.spectral_embedding needs of a projection.Spectral, with numpy's products."""

    def __init__(self, M, dd):
        self.M, self.dd, self.n, self.timings, self.calls = M, dd, M.shape[0], None, 0

    def mq(self, Q):
        self.calls += 1
        return self.M @ Q

    def degrees(self):
        return self.dd, 0

    def last_ms(self):
        return 0.0, 0.0, 0.25


@pytest.mark.parametrize("case", CASES)
def test_package_embedding_on_a_numpy_handle(case):
    from frisk_amd import projection as P
    g = G["cases"][case]
    _A, dd, M = host_matrix(case)
    h = NumpyHandle(M, dd)
    E, lam, res, it = P.spectral_embedding(h, g["k"], g["seed"])
    assert res.shape == lam.shape == (g["k"],) and res.max() <= P.SPECTRAL_TOL and it == h.calls < P.SPECTRAL_MAX_ITER
    assert np.all(np.diff(lam) <= 4 * EPS)                          # descending, up to the rounding of a Rayleigh quotient
    assert h.timings["products"] == it and h.timings["product_ms"] == 0.25 * it and h.timings["host_ms"] > 0
    check_embedding(case, E, lam, res, M, dd)
    big = np.argmax(np.abs(E), axis=0)
    assert np.all(E[big, np.arange(g["k"])] > 0)                    # sklearn's sign rule
    Eo, lo, _ro, ito = SO.embedding(M, dd, g["k"], g["seed"])
    assert it == ito and np.abs(E - Eo).max() <= 1e-13 * np.abs(Eo).max() and np.abs(lam - lo).max() <= 1e-14


def test_embedding_at_max_iter_warns_and_returns(caplog):
    from frisk_amd import projection as P
    _A, dd, M = host_matrix("close3")
    with caplog.at_level(logging.WARNING):
        E, lam, res, it = P.spectral_embedding(NumpyHandle(M, dd), 3, 0, max_iter=3)
    assert it == 3 and res.max() > P.SPECTRAL_TOL and E.shape == (150, 3) and "spectral embedding" in caplog.text


def test_constants_and_their_derivations():
    from frisk_amd import projection as P
    assert (P.SPECTRAL_MAX_K, P.SPECTRAL_MAX_P, P.SPECTRAL_GUARD, P.SPECTRAL_MAX_N) == (16, 26, 10, 50000)
    assert (P.SPECTRAL_TOL, P.SPECTRAL_MAX_ITER) == (SO.TOL, SO.MAX_ITER)
    assert P.SPECTRAL_TOL >= 8 * P.SPECTRAL_MAX_N * EPS                     # above the rounding floor of a product at the cap
    assert P.SPECTRAL_MAX_ITER >= np.log(1 / P.SPECTRAL_TOL) / -np.log(1.9 / 2.0)      # the worst contraction at gap 0.1


class _Stop(Exception):
    pass


def test_kmeans_draws_from_the_given_state(monkeypatch):
    """kmeans(..., rs=rs) seeds from rs itself, and after the n draws of v0 its first k-means++ picks are sklearn's"""
    from frisk_amd import projection as P
    for case in ("blobs3", "k16", "close3"):
        g = G["cases"][case]
        rs = np.random.RandomState(g["seed"])
        rs.uniform(-1, 1, g["n"])
        _c, idx = P.kmeans_plusplus(SO.array(case, "embedding"), g["k"], rs)
        # (the rows of one blob agree to 1e-10 where the blobs are far apart, and which of them a draw lands on hangs on the last
        # bits of the distances: there the picks are compared by blob, which the stream of draws decides)
        labels = SO.array(case, "labels")
        assert labels[idx].tolist() == labels[SO.array(case, "kpp")].tolist(), case
        assert case != "close3" or idx.tolist() == SO.array(case, "kpp").tolist()

    def stop(Y, k, rs):
        raise _Stop(rs)
    monkeypatch.setattr(P, "kmeans_plusplus", stop)
    E, mine = SO.array("blobs3", "embedding"), np.random.RandomState(77)
    with pytest.raises(_Stop) as e:
        P.kmeans(E, 3, seed=5, rs=mine)
    assert e.value.args[0] is mine
    with pytest.raises(_Stop) as e:
        P.kmeans(E, 3, seed=5)
    want, got = np.random.RandomState(5).get_state(), e.value.args[0].get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


def test_spectral_argument_errors():
    from frisk_amd import projection as P
    Y = np.random.RandomState(0).rand(20, 2)
    for k in (0, 17, 20, 21, -1):
        with pytest.raises(ValueError, match="n_clusters"):
            P.spectral(Y, k)
    with pytest.raises(ValueError, match="n_clusters"):
        P.spectral(Y[:2], 2)
    with pytest.raises(ValueError, match="between 2 and 50000 samples"):
        P.spectral(Y[:1], 1)
    with pytest.raises(ValueError, match="2-d"):
        P.spectral(Y[:, 0], 1)


# ------------------------------------------------------------------------------------------------ CLI and ABI
class Clock:
    def __init__(self):
        self.laps = []

    def lap(self, name):
        self.laps.append(name)


def _fake_pca(X, dims, device=0):
    from frisk_amd.projection import PCAResult
    return PCAResult(X[:, :dims].copy(), np.zeros((dims, X.shape[1])), np.ones(dims), np.zeros(X.shape[1]),
                     {"cov_ms": 0.0, "eigh_ms": 0.0, "transform_ms": 0.0})


@pytest.mark.parametrize("dump", [False, True])
def test_cli_dispatches_spectral_and_dumps_the_labels(tmp_path, monkeypatch, dump):
    from frisk_amd import cli, projection as P
    calls = []

    def spectral(Y, k, seed=0, device=0, **kw):
        calls.append((Y.shape, k, seed, device))
        labels = (np.arange(Y.shape[0]) % k).astype(np.int32)
        return P.SpectralResult(labels, np.zeros((Y.shape[0], k)), np.ones(k), np.zeros(k), 9, 0,
                                {"affinity_ms": 1.0, "normalise_ms": 1.0, "products_ms": 1.0, "products_wall_ms": 1.0,
                                 "host_ms": 1.0, "embedding_ms": 1.0, "kmeans_ms": 1.0})
    monkeypatch.setattr(P, "pca", _fake_pca)
    monkeypatch.setattr(P, "spectral", spectral)
    argv = ["-H", "x.fa", "-t", str(tmp_path), "--runProjection", "PCA", "--cluster", "SPECTRAL", "--kClusters", "3", "--seed", "5"]
    args = cli.build_parser().parse_args(argv + (["--dumpPCAdata"] if dump else []))
    clock = Clock()
    assert cli._project(args, np.random.RandomState(1).rand(11, 44), 0, clock) is None      # no labels: no cluster GFF3 follows
    assert calls == [((11, 2), 3, 5, 0)] and clock.laps == ["PCA", "SPECTRAL"]
    assert os.listdir(tmp_path) == (["anomSPECTRAL"] if dump else [])
    if dump:
        assert pickle.load(open(tmp_path / "anomSPECTRAL", "rb")).tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1]


def test_cli_goes_on_when_spectral_refuses(tmp_path, monkeypatch, caplog):
    from frisk_amd import cli, projection as P
    monkeypatch.setattr(P, "pca", _fake_pca)
    args = cli.build_parser().parse_args(["-H", "x.fa", "-t", str(tmp_path), "--runProjection", "PCA", "--cluster", "SPECTRAL",
                                          "--kClusters", "11", "--dumpPCAdata"])
    clock = Clock()
    with caplog.at_level(logging.WARNING):
        assert cli._project(args, np.random.RandomState(1).rand(11, 44), 0, clock) is None  # k >= n: refused before any device call
    assert "--cluster SPECTRAL skipped" in caplog.text and clock.laps == ["PCA"] and os.listdir(tmp_path) == []


def test_cli_after_nmf_runs_no_spectral(tmp_path, monkeypatch):
    from frisk_amd import cli, projection as P
    monkeypatch.setattr(P, "nmf", lambda X, dims, seed=0, device=0: P.NMFResult(
        X[:, :dims].copy(), None, 1, 1, [], None, None, {"init_ms": 0.0, "fit_ms": 0.0, "transform_ms": 0.0}))
    monkeypatch.setattr(P, "spectral", lambda *a, **k: pytest.fail("spectral after NMF"))
    args = cli.build_parser().parse_args(["-H", "x.fa", "-t", str(tmp_path), "--runProjection", "NMF", "--cluster", "SPECTRAL"])
    assert cli._project(args, np.random.RandomState(1).rand(11, 44), 0, Clock()) is None


def test_unavailable_is_unchanged_for_spectral():
    from frisk_amd.cli import CLUSTERINGS, CLUSTERINGS_UNWRITTEN, PROJECTIONS, build_parser, unavailable
    assert CLUSTERINGS_UNWRITTEN == ("SPECTRAL",) and "SPECTRAL" not in CLUSTERINGS
    for proj in PROJECTIONS + ("NMF", "SKL-TSNE"):
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", proj, "--cluster", "SPECTRAL"])
        assert unavailable(args) == [("cluster", "sklearn clustering is out of scope")]
    assert "CLUSTERINGS" in unavailable.__doc__ and "SPECTRAL" in unavailable.__doc__


def test_spectral_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    want = {"frisk_spectral_create", "frisk_spectral_affinity", "frisk_spectral_degrees", "frisk_spectral_matrix",
            "frisk_spectral_mq", "frisk_spectral_last_ms", "frisk_spectral_destroy"}
    assert want <= names
    root = os.path.join(os.path.dirname(__file__), "..")
    header = open(os.path.join(root, "include", "frisk_hip.h")).read()
    for name in want:
        assert name + "(" in header
    src = open(os.path.join(root, "frisk_amd", "csrc", "spectral_kernels.h")).read()
    assert "SPECTRAL_MAX_P = 26" in src and "SPECTRAL_MAX_K = 16" in src and "namespace frisk_spectral_impl" in src
    unit = open(os.path.join(root, "frisk_amd", "csrc", "frisk_analysis.hip")).read()
    assert unit.index('"nmf_kernels.h"') < unit.index('"spectral_kernels.h"')


# ------------------------------------------------------------------------------------------------ C_EXP
def test_c_exp_is_the_calibrated_constant():
    """the worst error of numpy's double exp, in units of eps64, over the exponents of every golden case; the next power of two,
    times 4"""
    worst = 0.0
    for case in CASES:
        x = -G["cases"][case]["gamma"] * SO.sqdist(SO.array(case, "Y"))
        worst = max(worst, float(HP.exp_ratio(x).max()))
    print("worst exp ratio %.4f -> C_EXP %.1f" % (worst, HP.calibrate(worst)))
    assert 0.0 < worst <= 1.0, worst            # a faithfully rounded exp; recorded in spectral_oracle_hp: 0.580
    assert HP.calibrate(worst) <= HP.C_EXP == 4.0


def test_hp_oracle_agrees_with_the_double_oracle():
    for case in ("d5", "isolated", "minus_one"):
        g = G["cases"][case]
        Y = SO.array(case, "Y")
        A_hp, d2 = HP.affinity(Y, g["gamma"])
        A = SO.affinity(Y, g["gamma"])
        assert np.all(np.abs(A - A_hp.astype(np.float64)) <= HP.affinity_bound(A_hp, d2, g["d"], g["gamma"]))
        w = HP.degrees(A_hp).astype(np.float64)
        assert int(np.sum(w == 0)) == g["n_isolated"]
