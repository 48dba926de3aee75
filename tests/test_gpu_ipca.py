"""IncrementalPCA on the GPU (csrc/ipca_kernels.h through frisk_amd.projection.IncrementalPCA / incremental_pca) against sklearn's
recorded states (tests/golden/ipca, tools/make_golden_ipca.py): every batch started from sklearn's state of the batch before and
chained from the start, the full fit bit for bit equal to chained partial_fit calls and from run to run, the distance from the PCA
of X (an alias of pca() fails), the argument checks of the C ABI, rows outside the fit, one run at n = 30 000, F = 2 772 against
tests/ipca_oracle.py, and the CLI end to end.

Tolerances (tests/ipca_oracle.py): Y and components 1e-9 of max|golden|, scalars 1e-9 relative, noise_variance_ 1e-9 of
explained_variance_[0]; a component whose recorded sign margin is below 1e-6 is compared up to sign.  Every test prints its worst
ratio to the tolerance before it asserts."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ipca_oracle as IO
from golden_util import GOLD, INPUTS

pytestmark = pytest.mark.gpu

G = IO.G
CASES = sorted(G["cases"])
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _state(fit):
    n, mean, var, S, Vt = fit.state()
    return {"n": n, "mean": mean, "var": var, "S": S, "Vt": Vt, "ev": fit.explained_variance_, "evr": fit.explained_variance_ratio_,
            "noise": fit.noise_variance_}


def _merge(worst, r):
    for key, v in r.items():
        worst[key] = max(worst.get(key, 0.0), v)


# ------------------------------------------------------------------------------------------------ states
@pytest.mark.parametrize("case", CASES)
def test_batches_match_sklearn_states(case):
    """after each batch, from sklearn's recorded state of the batch before (set through the handle) and chained from the start"""
    from frisk_amd.projection import IncrementalPCA
    g, a = G["cases"][case], IO.arrays(case)
    X = IO.X_of(case)
    worst = {}
    with IncrementalPCA(g["F"], g["d"]) as stepped, IncrementalPCA(g["F"], g["d"]) as chained:
        lo = seen = 0
        for k, b in enumerate(g["batch_sizes"]):
            Xb = X[lo:lo + b]
            want = IO.state_of(a, k, seen + b)
            if k:
                prev = IO.state_of(a, k - 1, seen)
                stepped.set_state(seen, prev["mean"], prev["var"], prev["S"], prev["Vt"])
            for fit in (stepped, chained):
                fit.partial_fit(Xb)
                assert fit.n_samples_seen_ == seen + b == fit.state()[0]
                r, s = IO.ratios(_state(fit), want, a["sign_margin"][k])
                _merge(worst, r)
            lo, seen = lo + b, seen + b
        for fit in (stepped, chained):
            r, s = IO.ratios(_state(fit), want, a["sign_margin"][-1])
            _merge(worst, {"Y": IO.y_ratio(fit.transform(X), a["Y"], s)})
    print("%s: worst |GPU - sklearn| / tolerance: %s" % (case, {k: "%.3g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", CASES)
def test_full_fit_equals_chained_batches_and_repeats_bit_for_bit(case):
    from frisk_amd.projection import IncrementalPCA, incremental_pca
    g, a = G["cases"][case], IO.arrays(case)
    X = IO.X_of(case)
    r1 = incremental_pca(X, g["d"], batch_size=g["batch_size"])
    r2 = incremental_pca(X, g["d"], batch_size=g["batch_size"])
    assert r1.batch_sizes == g["batch_sizes"] and r1.n_samples_seen_ == g["n"]
    with IncrementalPCA(g["F"], g["d"]) as fit:
        lo = 0
        for b in g["batch_sizes"]:
            fit.partial_fit(X[lo:lo + b])
            lo += b
        st, Y = _state(fit), fit.transform(X)
    for r in (r1, r2):
        assert r.Y.tobytes() == Y.tobytes()
        for got, want in ((r.mean_, st["mean"]), (r.var_, st["var"]), (r.singular_values_, st["S"]), (r.components_, st["Vt"]),
                          (r.explained_variance_, st["ev"]), (r.explained_variance_ratio_, st["evr"])):
            assert got.tobytes() == want.tobytes()
        assert r.noise_variance_ == st["noise"]
    assert set(r1.timings) >= {"stats_gram_ms", "eigh_ms", "transform_ms"}
    rr, s = IO.ratios(st, IO.state_of(a, len(g["batch_sizes"]) - 1, g["n"]), a["sign_margin"][-1])
    rr["Y"] = IO.y_ratio(r1.Y, a["Y"], s)
    print("%s: worst |GPU - sklearn| / tolerance of the full fit: %s" % (case, {k: "%.3g" % v for k, v in rr.items()}))
    assert max(rr.values()) <= 1.0, rr


@pytest.mark.parametrize("case", CASES)
def test_distance_from_the_pca_of_X(case):
    """multi-batch: farther than 1e-6 max|Y| from pca(X, d).Y up to sign (an alias of pca() fails here); one batch: the same fit"""
    from frisk_amd.projection import incremental_pca, pca
    g = G["cases"][case]
    X = IO.X_of(case)
    Y, Yp = incremental_pca(X, g["d"], batch_size=g["batch_size"]).Y, pca(X, g["d"]).Y
    dist = IO.distance_up_to_sign(Y, Yp)
    print("%s: %d batches, |Y - Y_PCA| / max|Y| up to sign = %.3g (recorded with sklearn: %.3g)"
          % (case, len(g["batch_sizes"]), dist, g["pca_distance"]))
    if len(g["batch_sizes"]) > 1:
        assert dist > 1e-6
    else:
        assert dist <= IO.TOL


def test_transform_of_rows_outside_the_fit():
    from frisk_amd.projection import IncrementalPCA
    g, a = G["cases"]["multi44"], IO.arrays("multi44")
    X = IO.X_of("multi44")
    st = IO.state_of(a, len(g["batch_sizes"]) - 1, g["n"])
    new = IO.make_X({"n": 333, "orders": g["X"]["orders"], "spread": 40.0, "seed": 99})
    with IncrementalPCA(g["F"], g["d"]) as fit:
        with pytest.raises(Exception):
            fit.transform(new)                      # nothing fitted yet
        fit.set_state(g["n"], st["mean"], st["var"], st["S"], st["Vt"])
        Y = fit.transform(new)
        assert fit.transform(new[:1]).tobytes() == Y[:1].tobytes() and fit.transform(new[7:200]).tobytes() == Y[7:200].tobytes()
        assert fit.transform(new[:0]).shape == (0, g["d"])
    ratio = IO.y_ratio(Y, IO.transform(new, st))
    print("transform of 333 new rows: worst ratio %.3g" % ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ C ABI
def test_abi_rejects_bad_input():
    from frisk_amd import _ffi
    from frisk_amd.projection import IncrementalPCA, incremental_pca
    L = _ffi.lib()
    E, ST = _ffi.E_ARG, _ffi.E_STATE
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    X = np.random.RandomState(0).rand(20, 5)
    G5, Y = np.empty((5, 5)), np.empty((20, 2))
    h = C.c_void_p()
    assert L.frisk_ipca_create(0, 5, 2, None) == E
    assert L.frisk_ipca_create(0, 5, 0, C.byref(h)) == E and not h          # d < 1
    assert L.frisk_ipca_create(0, 5, 6, C.byref(h)) == E and not h          # d > f
    assert L.frisk_ipca_create(0, 0, 1, C.byref(h)) == E and not h
    assert L.frisk_ipca_gram(None, p(X), 20, p(G5)) == E
    assert L.frisk_ipca_create(0, 5, 2, C.byref(h)) == _ffi.OK and h
    try:
        assert L.frisk_ipca_gram(h, None, 20, p(G5)) == E
        assert L.frisk_ipca_gram(h, p(X), 20, None) == E
        assert L.frisk_ipca_gram(h, p(X), 0, p(G5)) == E                    # b < 1
        assert L.frisk_ipca_gram(h, p(X), 1, p(G5)) == E                    # a first batch with b < d
        for v in (np.nan, np.inf):
            bad = X.copy()
            bad[3, 1] = v
            assert L.frisk_ipca_gram(h, p(bad), 20, p(G5)) == E
        S, Vt = np.ones(2), np.eye(5)[:2].copy()
        assert L.frisk_ipca_commit(h, p(S), p(Vt)) == ST                    # no batch is pending
        assert L.frisk_ipca_transform(h, p(X), 20, p(Y)) == ST              # nothing fitted
        assert L.frisk_ipca_get(h, None, p(np.empty(5)), None, None, None) == ST
        assert L.frisk_ipca_gram(h, p(X), 20, p(G5)) == _ffi.OK
        assert np.array_equal(G5, G5.T) and np.isfinite(G5).all()
        assert L.frisk_ipca_commit(h, None, p(Vt)) == E and L.frisk_ipca_commit(h, p(S), None) == E
        assert L.frisk_ipca_commit(h, p(np.array([1.0, np.nan])), p(Vt)) == E
        assert L.frisk_ipca_commit(h, p(S), p(Vt)) == _ffi.OK
        assert L.frisk_ipca_commit(h, p(S), p(Vt)) == ST
        seen = C.c_int64()
        assert L.frisk_ipca_get(h, C.byref(seen), None, None, None, None) == _ffi.OK and seen.value == 20
        assert L.frisk_ipca_gram(h, p(X), 1, p(G5)) == _ffi.OK              # a later batch may be shorter than d
        assert L.frisk_ipca_transform(h, None, 20, p(Y)) == E and L.frisk_ipca_transform(h, p(X), 20, None) == E
        assert L.frisk_ipca_transform(h, p(X), 0, p(Y)) == E and L.frisk_ipca_transform(h, p(bad), 20, p(Y)) == E
        assert L.frisk_ipca_transform(h, p(X), 20, p(Y)) == _ffi.OK and np.isfinite(Y).all()
        assert L.frisk_ipca_set(h, -1, None, None, None, None) == E
        assert L.frisk_ipca_set(h, 5, None, p(np.ones(5)), p(S), p(Vt)) == E
        assert L.frisk_ipca_set(h, 5, p(np.full(5, np.nan)), p(np.ones(5)), p(S), p(Vt)) == E
        assert L.frisk_ipca_set(h, 0, None, None, None, None) == _ffi.OK
        assert L.frisk_ipca_transform(h, p(X), 20, p(Y)) == ST
        assert L.frisk_ipca_last_ms(h, 3) == -1.0 and L.frisk_ipca_last_ms(h, 1) >= 0.0
    finally:
        L.frisk_ipca_destroy(h)
    with pytest.raises(ValueError):
        IncrementalPCA(5, 6)                        # dims > F
    with pytest.raises(ValueError):
        incremental_pca(X, 6)
    with pytest.raises(ValueError):
        incremental_pca(X[:3], 4)                   # dims > the first batch's rows
    with pytest.raises(ValueError):
        incremental_pca(X, 3, batch_size=2)


# ------------------------------------------------------------------------------------------------ size
def test_thirty_thousand_rows_against_the_oracle():
    """n = 30 000, F = 2 772, d = 2: three batches (13 860, 13 860, 2 280), every state and Y against tests/ipca_oracle.py."""
    from frisk_amd.projection import incremental_pca, IncrementalPCA
    n, f, d = 30000, 2772, 2
    rs = np.random.RandomState(31)
    centres = rs.dirichlet(np.full(f, 2.0), size=3)
    X = rs.standard_gamma(centres[rs.randint(0, 3, n)] * 200.0 + 1e-3)
    X /= X.sum(axis=1, keepdims=True)
    res = incremental_pca(X, d)
    assert res.batch_sizes == [13860, 13860, 2280]
    worst, st, lo = {}, None, 0
    with IncrementalPCA(f, d) as fit:
        for b in res.batch_sizes:
            fit.partial_fit(X[lo:lo + b])
            st = IO.partial_fit(st, X[lo:lo + b], d)
            assert st["gap"] >= G["min_gap"]
            r, s = IO.ratios(_state(fit), st, _margin(st["Vt"]))        # the oracle's own sign margins
            _merge(worst, r)
            lo += b
        assert fit.state()[4].tobytes() == res.components_.tobytes()
    _merge(worst, {"Y": IO.y_ratio(res.Y, IO.transform(X, st), s)})
    print("n 30000, F 2772: worst |GPU - oracle| / tolerance: %s; timings %s"
          % ({k: "%.3g" % v for k, v in worst.items()}, {k: round(v, 1) for k, v in res.timings.items()}))
    assert max(worst.values()) <= 1.0, worst


def _margin(comps):
    a = np.sort(np.abs(comps), axis=1)
    return (a[:, -1] - a[:, -2]) / a[:, -1]


# ------------------------------------------------------------------------------------------------ CLI
def _cli(tmp, argv, fasta):
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, fasta), "-t", str(tmp)] + argv
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


@pytest.mark.parametrize("tag", sorted(G["e2e"]))
def test_cli_incremental_pca_dbscan_writes_both_gffs(tmp_path, tag):
    """--runProjection IncrementalPCA --cluster DBSCAN on the fixture (--pcaMax 3: one batch; --pcaMax 2: batches 60, 60, 60, 18):
    the reference's cluster GFF3 byte for byte; a.gff3 of the unmerged anomalous windows equal to the reference's in every field,
    its KLD value to 1e-11 (the CLI prints the score table's 12 significant digits, the reference 17: the scan's text, pinned by
    the other CLI tests of this fixture, not this projection's); and, since DBSCAN's partition here is the same for PCA and
    IncrementalPCA, the dumped anomCounts through incremental_pca against sklearn's recorded Y."""
    from frisk_amd.projection import incremental_pca, pca
    e = G["e2e"][tag]
    a = np.load(os.path.join(GOLD, "ipca", e["file"]))
    out = tmp_path / tag
    p = _cli(out, e["argv"] + ["--dumpPCAdata"], e["fasta"])
    assert "IncrementalPCA of %d x %d k-mer proportions in %d batches" % (e["n_anomalous"], e["F"], len(e["batch_sizes"])) in p.stderr
    assert "not available" not in p.stderr and "is not built here" not in p.stderr
    assert sorted(os.listdir(out)).count(e["cluster_gff_name"]) == 1
    assert open(out / e["cluster_gff_name"]).read() == e["cluster_gff"]
    got = open(out / "a.gff3").read().splitlines()
    want = e["anomaly_gff"].splitlines()
    assert len(got) == len(want) == e["n_anomalous"] + 1 and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        gf, wf = g.split("\t"), w.split("\t")
        assert gf[:8] == wf[:8]
        gid, gk = gf[8].split(";")
        wid, wk = wf[8].split(";")
        assert gid == wid and gk.startswith("KLD=") and abs(float(gk[4:]) - float(wk[4:])) <= 1e-11
    with open(out / "anomCounts", "rb") as fh:
        anomCounts = pickle.load(fh)
    assert IO.sha(anomCounts) == e["anomCounts_sha256"]
    r = incremental_pca(anomCounts, 2)
    assert r.batch_sizes == e["batch_sizes"]
    st = {"n": r.n_samples_seen_, "mean": r.mean_, "var": r.var_, "S": r.singular_values_, "Vt": r.components_,
          "ev": r.explained_variance_, "evr": r.explained_variance_ratio_, "noise": r.noise_variance_}
    rr, s = IO.ratios(st, IO.state_of(a, len(e["batch_sizes"]) - 1, e["n_anomalous"]), a["sign_margin"][-1])
    rr["Y"] = IO.y_ratio(r.Y, a["Y"], s)
    dist = IO.distance_up_to_sign(r.Y, pca(anomCounts, 2).Y)
    print("%s: worst |GPU - sklearn| / tolerance: %s; distance from PCA %.3g" % (tag, {k: "%.3g" % v for k, v in rr.items()}, dist))
    assert max(rr.values()) <= 1.0, rr
    assert dist > 1e-6 if len(e["batch_sizes"]) > 1 else dist <= IO.TOL


def test_cli_incremental_pca_kmeans_writes_its_gff(tmp_path):
    e = G["e2e"]["pcamax2"]
    out = tmp_path / "K"
    argv = e["argv"][:e["argv"].index("--cluster")] + ["--cluster", "KMEANS", "--gffOutfile", "a.gff3"]
    p = _cli(out, argv, e["fasta"])
    assert "not available" not in p.stderr
    text = open(out / e["kmeans_gff_name"]).read()
    assert text.count("\n") == e["n_anomalous"] + text.startswith("##gff-version")
