"""PY-TSNE without a GPU: the numpy restatement (tests/tsne_oracle.py) against the reference's own states recorded in
tests/golden/tsne (tools/make_golden_tsne.py), the exact 4 q form of the exaggerated P, the CLI's mapping of PY-TSNE to a built
projection and the declared C ABI."""
import json
import os

import numpy as np
import pytest

import tsne_oracle as TO
from golden_util import GOLD

G = json.load(open(os.path.join(GOLD, "tsne.json")))
CASES = sorted(G["cases"])


def A(case):
    return np.load(os.path.join(GOLD, "tsne", G["cases"][case]["file"]))


@pytest.mark.parametrize("case", CASES)
def test_oracle_affinities_match_reference(case):
    g, a = G["cases"][case], A(case)
    beta, tries, q = TO.affinities(a["Xp"], g["perplexity"])
    assert tries.tolist() == a["tries"].tolist()
    assert np.all(np.abs(beta - a["beta"]) <= 1e-12 * np.abs(a["beta"]))
    if "q" in a:
        qg = a["q"]
        clamped = qg == TO.Q_FLOOR
        assert np.array_equal(q == TO.Q_FLOOR, clamped)
        tol = TO.q_tolerance(a["Xp"], a["beta"])
        assert np.all((np.abs(q - qg) <= tol * qg)[~clamped])


@pytest.mark.parametrize("case", CASES)
def test_oracle_steps_match_reference_snapshots(case):
    """For every recorded t: the oracle's step t -> t + 1 from the reference's state lies within its bound of the reference's
    state at t + 1, with the gains equal wherever the sign of dY is decided."""
    g, a = G["cases"][case], A(case)
    q = a["q"] if "q" in a else TO.affinities(a["Xp"], g["perplexity"])[2]
    skipped = total = 0
    for t in g["snapshots"]:
        st = TO.step(a["Y_%d" % t], a["iY_%d" % t], a["gains_%d" % t], q, t, q_rel=1e-12)
        ok, skip = TO.compare_state(st, a["Y_%d" % (t + 1)], a["iY_%d" % (t + 1)], a["gains_%d" % (t + 1)])
        assert ok.all(), (t, np.argwhere(~ok)[:5].tolist())
        if st.cost is not None:
            assert abs(st.cost - a["cost"][(t + 1) // 10 - 1]) <= 1e-9 * abs(st.cost)
        skipped += skip
        total += ok.size
    assert skipped <= max(2, total // 1000)


def test_exaggerated_p_is_four_q_bit_for_bit():
    a = A("blobs3")
    assert np.array_equal(a["P0"], 4.0 * a["q"])
    assert np.array_equal(a["P0"] / 4.0, a["q"])
    assert np.array_equal(a["q"], np.maximum(a["P0"] / 4.0, TO.Q_FLOOR))
    assert (a["q"] == TO.Q_FLOOR).any()


def test_golden_costs_and_ensembles_are_sane():
    for case, g in G["cases"].items():
        cost = A(case)["cost"]
        assert cost.shape == (100,) and np.isfinite(cost).all()
        assert cost[-1] == g["ensemble_final_cost"][0]


def test_cli_maps_py_tsne_to_a_built_projection():
    from frisk_amd import postprocess as pp
    from frisk_amd.cli import PROJECTIONS, build_parser, unavailable
    assert "PY-TSNE" in PROJECTIONS and "SKL-TSNE" not in PROJECTIONS
    for clust in ("DBSCAN", "KMEANS"):
        args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "PY-TSNE", "--cluster", clust])
        assert unavailable(args) == []
    args = build_parser().parse_args(["-H", "x.fa", "--runProjection", "SKL-TSNE", "--cluster", "DBSCAN"])
    assert ("cluster", "sklearn clustering is out of scope") in unavailable(args)
    args = build_parser().parse_args(G["e2e"]["argv"][:-2] + ["-H", "x.fa", "--gffOutfile", "a.gff3"])
    assert pp.clusterGffName(args) == G["e2e"]["cluster_gff_name"]


def test_tsne_abi_is_declared():
    from frisk_amd import _ffi
    names = {n for n, _, _ in _ffi.SYMBOLS}
    assert {"frisk_tsne_create", "frisk_tsne_affinities", "frisk_tsne_run", "frisk_tsne_get", "frisk_tsne_set",
            "frisk_tsne_destroy"} <= names
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "frisk_hip.h")).read()
    for name in names:
        if name.startswith("frisk_tsne"):
            assert name + "(" in header
