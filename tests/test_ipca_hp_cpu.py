"""The per-entry IncrementalPCA pin without a GPU: tests/golden/ipca_hp.json regenerated (the float64 restatement of
tests/ipca_oracle.py against the long-double oracle of tests/ipca_oracle_hp.py, in forward-error units), the oracle's distance from
50-digit mpmath, the seven planted defects against the comparison the GPU test uses, the share of the correction row and of the
variance's cross term in the unpermuted cases, and the oracle against two recorded sklearn states."""
import numpy as np
import pytest

import ipca_hp_cases as K
import ipca_oracle as IO
import ipca_oracle_hp as HP

G = K.golden()
TOL = G["tolerance"]


def test_case_list_holds_the_shapes_it_is_for():
    ids = set(K.BY_ID)
    assert set(G["cases"]) == ids
    first = {(c.b, c.f, c.d) for c in K.CASES if c.seen == 0}
    assert {(b, 9, 2) for b in (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4033)} | {(1, 9, 1), (12, 5, 5)} <= first
    assert {(40, f, min(f, 2)) for f in (1, 2, 63, 64, 65, 255, 256, 257)} <= first
    assert {(b, 2772, 2) for b in (48, 49, 64, 65)} | {(b, 8, 2) for b in (32752, 32768, 32769)} <= first
    later = {(c.d + c.b + 1, c.b, c.f, c.d) for c in K.CASES if c.seen}
    assert {r for r, _b, f, d in later if (f, d) == (9, 2)} == {16, 17, 32, 33}
    assert (5, 1, 9, 3) in later and {d for _r, _b, f, d in later if f == 70} == {1, 2, 3, 64}
    assert (43, 40, 257, 2) in later and (64, 61, 2772, 2) in later
    for group in {c.group for c in K.CASES}:
        fams = {c.family for c in K.CASES if c.group == group}
        seen = {c.seen for c in K.CASES if c.group == group}
        assert fams >= {"kmer", "offset", "zeroconst", "sspan"}, group
        assert seen == ({0} if group.startswith("first") else set(K.SEEN)) and (group.startswith("first") or "unperm" in fams)
    cols = K.sample_cols(2772)
    assert len(cols) == len(set(cols.tolist())) == 48 and {0, 2771, 63, 64, 2751, 2752} <= set(cols.tolist())
    # the K split of State::gram at the shapes the list is for: (ksplit before the cap, rows_pad / 16)
    assert [(-(-b // 16)) for b in (32752, 32768, 32769)] == [2047, 2048, 2049]
    for cid in ("first_b/b64_f9_d2/zeroconst", "later_d/b20_f70_d64_seen7/zeroconst"):
        i = K.inputs(cid)
        assert not i.Xb[:, 0].any() and (i.Xb[:, -1] == 0.25).all()
    i = K.inputs("later_rows/b13_f9_d2_seen1/sspan")
    assert i.state["S"].tolist() == [1e3, 1e-3] and np.allclose(i.Vt_new @ i.Vt_new.T, np.eye(2), atol=1e-14)
    x = K.inputs("first_b/b129_f9_d2/offset").Xb
    assert abs(x.mean() - 1.0) < 1e-6 and 5e-7 < x.std() < 2e-6


def test_recorded_ratios_regenerate_and_the_tolerance_is_eight_times_the_worst():
    """mean and var are numpy's own sums (one order): equal to the recorded figures; G and Y go through BLAS, whose summation
    order may differ between builds: within a factor of two of the record, and within the tolerance."""
    assert G["factor"] == K.FACTOR == 8 and G["quantities"] == list(K.QUANTITIES) and G["unit_eps"] == 2.0 ** -52
    worst = dict.fromkeys(K.QUANTITIES, 0.0)
    for c in K.CASES:
        r = K.check(c.id, K.restate(c.id), TOL, what="float64 restatement")
        for q in K.QUANTITIES:
            worst[q] = max(worst[q], r[q])
            if q in ("mean", "var"):
                assert r[q] == G["cases"][c.id][q], (c.id, q)
    print("worst |restatement - oracle| / unit: %s; recorded %s" % (worst, G["worst"]))
    for q in K.QUANTITIES:
        assert G["worst"][q] == max(v[q] for v in G["cases"].values())
        assert TOL[q] == 8 * G["worst"][q] and 0 < TOL[q] < 1e3     # (a few hundred roundings, not a chosen number)
        assert G["worst"][q] / 2 <= worst[q] <= G["worst"][q] * 2


def test_planted_none_is_the_restatement_bit_for_bit():
    for cid in ("first_b/b17_f9_d2/kmer", "later_rows/b14_f9_d2_seen7/unperm", "later_d/b20_f70_d64_seen100000/sspan"):
        i = K.inputs(cid)
        mean, var, T, A = K._planted(i.Xb, i.state, None)
        m2, v2, T2 = IO.mean_var_update(i.Xb, 0 if i.state is None else i.state["n"], *(
            (None, None) if i.state is None else (i.state["mean"], i.state["var"])))
        assert mean.tobytes() == m2.tobytes() and var.tobytes() == v2.tobytes() and T.tobytes() == T2.tobytes()
        assert A.tobytes() == IO.stacked(i.Xb, i.state, m2, T2).tobytes()


@pytest.mark.parametrize("defect", K.DEFECTS)
def test_comparison_rejects_a_planted_defect(defect):
    """check(), which the GPU test calls, rejects the defect, and by at least 10 x the tolerance of a quantity on some case."""
    best, rejected = (0.0, None, None), 0
    for c in K.CASES:
        got = K.restate(c.id, defect)
        for q, v in K.compare(c.id, got).items():
            if v / TOL[q] > best[0]:
                best = (v / TOL[q], q, c.id)
        try:
            K.check(c.id, got, TOL, what=defect)
        except AssertionError:
            rejected += 1
    rec = G["defects"][defect]
    print("%s: rejected on %d of %d cases; worst %.3g x the tolerance of %s on %s" % ((defect, rejected, len(K.CASES)) + best))
    assert rejected and best[0] >= K.DEFECT_MARGIN
    assert max(v["ratio_over_tolerance"] for v in rec.values()) >= K.DEFECT_MARGIN
    assert all(v["case"] in K.BY_ID for v in rec.values() if v["case"])


def test_unpermuted_batches_load_the_correction_row_and_the_cross_term():
    corr, cross = K.assert_shares(0.10)
    print("correction row: %.3g of trace G (%s); cross term: %.3g of var (%s)" % (corr + cross))
    assert G["shares"]["correction_row_of_trace_G"]["case"] == corr[1] and G["shares"]["cross_term_of_var"]["case"] == cross[1]
    # and a permuted batch does not: the gap the unpermuted family closes
    assert K.oracle("later_rows/b29_f9_d2_seen100000/kmer")["corr_share"] < corr[0]


def test_oracle_is_far_closer_to_mpmath_than_the_tolerance():
    mp = pytest.importorskip("mpmath")
    assert mp and set(G["oracle_vs_mpmath"]) == set(K.MP_CASES) and any(K.BY_ID[c].seen for c in K.MP_CASES)
    for cid in K.MP_CASES:
        i = K.inputs(cid)
        st = i.state or {"n": 0, "mean": None, "var": None, "S": None, "Vt": None}
        d = HP.distance_from_mp(i.Xb, st["n"], st["mean"], st["var"], st["S"], st["Vt"], i.Vt_new)
        print("%s: |oracle - mpmath| / unit %s" % (cid, d))
        for q in K.QUANTITIES:
            assert d[q] <= 2.0 ** -11 and d[q] == pytest.approx(G["oracle_vs_mpmath"][cid][q], rel=1e-6, abs=1e-12)
            assert 1000 * d[q] <= TOL[q]


@pytest.mark.parametrize("case,k", [("multi44", 0), ("multi44_d3", 1)])
def test_oracle_reproduces_a_recorded_sklearn_state(case, k):
    """mean and var of batch k from sklearn's state before it, within tests/ipca_oracle.py's tolerance; and G: its top d
    eigenpairs are sklearn's singular values and components."""
    g, a = IO.G["cases"][case], IO.arrays(case)
    X = IO.X_of(case)
    lo = sum(g["batch_sizes"][:k])
    b = g["batch_sizes"][k]
    prev = IO.state_of(a, k - 1, lo) if k else {"n": 0, "mean": None, "var": None, "S": None, "Vt": None}
    want = IO.state_of(a, k, lo + b)
    o = HP.batch(X[lo:lo + b], prev["n"], prev["mean"], prev["var"], prev["S"], prev["Vt"])
    Gm = o["G"].astype(np.float64)
    w, v = np.linalg.eigh((Gm + Gm.T) / 2)
    order = np.argsort(w, kind="stable")[::-1][:g["d"]]
    got = {"mean": o["mean"].astype(np.float64), "var": o["var"].astype(np.float64), "S": np.sqrt(w[order]),
           "Vt": IO.sign_rule(v[:, order].T.copy())}
    got["ev"] = got["S"] ** 2 / (lo + b - 1)
    got["evr"] = got["S"] ** 2 / np.sum(got["var"] * (lo + b))
    got["noise"] = want["noise"]
    r, _s = IO.ratios(got, want, a["sign_margin"][k])
    print("%s batch %d: worst |oracle - sklearn| / tolerance: %s" % (case, k, {q: "%.2g" % x for q, x in r.items()}))
    assert max(r.values()) <= 1.0, r
