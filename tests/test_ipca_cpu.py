"""IncrementalPCA without a GPU: the CLI's mapping of IncrementalPCA to a built projection, the declared C ABI, the batch rule
against recorded sklearn.utils.gen_batches outputs, the goldens of tools/make_golden_ipca.py (regenerated inputs and their hashes,
the recorded caps), and the numpy restatement of the Gram route (tests/ipca_oracle.py) against every recorded sklearn state."""
import os

import numpy as np
import pytest

import ipca_oracle as IO

G = IO.G
CASES = sorted(G["cases"])


# ------------------------------------------------------------------------------------------------ CLI and ABI
def test_cli_maps_incremental_pca_to_a_built_projection():
    from frisk_amd import postprocess as pp
    from frisk_amd.cli import PROJECTIONS, build_parser, unavailable
    assert "IncrementalPCA" in PROJECTIONS
    for clust in ("DBSCAN", "KMEANS"):
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "IncrementalPCA", "--cluster", clust])
        assert unavailable(args) == []
    args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "IncrementalPCA", "--cluster", "SPECTRAL"])
    assert ("cluster", "sklearn clustering is out of scope") in unavailable(args)
    for proj in ("NMF", "SKL-TSNE"):            # the methods still not built keep their behaviour
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", proj, "--cluster", "DBSCAN"])
        assert proj not in PROJECTIONS and ("cluster", "sklearn clustering is out of scope") in unavailable(args)
    for e in G["e2e"].values():
        args = build_parser().parse_args(e["argv"] + ["-H", "x.fa"])
        assert pp.clusterGffName(args) == e["cluster_gff_name"] == "IncrementalPCA_DBSCAN_k_2_cluster_labeled_windows_a.gff3"
        args = build_parser().parse_args(e["argv"][:-6] + ["--cluster", "KMEANS", "-H", "x.fa", "--gffOutfile", "a.gff3"])
        assert pp.clusterGffName(args) == e["kmeans_gff_name"]


def test_ipca_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    want = {"frisk_ipca_create", "frisk_ipca_gram", "frisk_ipca_commit", "frisk_ipca_get", "frisk_ipca_set",
            "frisk_ipca_transform", "frisk_ipca_last_ms", "frisk_ipca_destroy"}
    assert want <= names
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "frisk_hip.h")).read()
    for name in want:
        assert name + "(" in header


# ------------------------------------------------------------------------------------------------ batch rule
def test_batch_rule_matches_recorded_gen_batches():
    from frisk_amd.projection import gen_batches
    assert len(G["gen_batches"]) >= 15
    for c in G["gen_batches"]:
        for rule in (gen_batches, IO.gen_batches):
            got = rule(c["n"], c["batch_size"], c["min_batch_size"])
            assert [hi - lo for lo, hi in got] == c["sizes"], c
            assert got[0][0] == 0 and got[-1][1] == c["n"] and all(a[1] == b[0] for a, b in zip(got, got[1:]))
    by = {(c["n"], c["batch_size"], c["min_batch_size"]): c["sizes"] for c in G["gen_batches"]}
    assert by[(223, 220, 2)] == [220, 3] and by[(221, 220, 2)] == [221]         # a tail of d rows stays, a shorter one is merged
    assert by[(150, 220, 2)] == [150] and by[(440, 220, 2)] == [220, 220]       # n < batch, n a multiple
    assert by[(30000, 13860, 2)] == [13860, 13860, 2280]


# ------------------------------------------------------------------------------------------------ goldens
@pytest.mark.parametrize("case", CASES)
def test_golden_inputs_regenerate_and_meet_the_caps(case):
    g, a = G["cases"][case], IO.arrays(case)
    X = IO.X_of(case)
    assert X.shape == (g["n"], g["F"])
    size = 5 * g["F"] if g["batch_size"] is None else g["batch_size"]
    assert [hi - lo for lo, hi in IO.gen_batches(g["n"], size, g["d"])] == g["batch_sizes"]
    nb = len(g["batch_sizes"])
    assert a["noise"].shape == (nb,) and a["sign_margin"].shape == (nb, g["d"]) and a["Y"].shape == (g["n"], g["d"])
    assert a["comps_%d" % (nb - 1)].shape == (g["d"], g["F"]) and "comps_%d" % nb not in a.files
    assert g["gap"] >= G["min_gap"]
    assert nb == 1 or g["pca_distance"] >= G["min_pca_distance"]
    assert g["min_sign_margin"] == float(a["sign_margin"].min())


def _case_ratios(X, g, a):
    """Worst tolerance ratios of the oracle, each batch started from sklearn's recorded state of the batch before, and chained."""
    worst = {}
    lo, st_chain, seen = 0, None, 0
    for k, b in enumerate(g["batch_sizes"]):
        Xb = X[lo:lo + b]
        want = IO.state_of(a, k, seen + b)
        for st in ((None if k == 0 else IO.state_of(a, k - 1, seen)), st_chain):
            got = IO.partial_fit(st, Xb, g["d"])
            r, s = IO.ratios(got, want, a["sign_margin"][k])
            for key, v in r.items():
                worst[key] = max(worst.get(key, 0.0), v)
        st_chain = got
        lo, seen = lo + b, seen + b
    worst["Y"] = IO.y_ratio(IO.transform(X, st_chain), a["Y"], s)
    return worst


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_every_sklearn_state(case):
    g, a = G["cases"][case], IO.arrays(case)
    worst = _case_ratios(IO.X_of(case), g, a)
    print("%s: worst |oracle - sklearn| / tolerance: %s" % (case, {k: "%.2g" % v for k, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", CASES)
def test_multi_batch_fit_is_not_the_pca(case):
    g, a = G["cases"][case], IO.arrays(case)
    dist = IO.distance_up_to_sign(a["Y"], IO.pca_Y(IO.X_of(case), g["d"]))
    if len(g["batch_sizes"]) > 1:
        assert dist > 1e-6
    else:
        assert dist <= IO.TOL
