"""The extended-precision MDS pin without a GPU: tests/golden/mds_hp.json re-derived (input hashes, the float64 model of
tests/mds_oracle.py against the long-double oracle of tests/mds_oracle_hp.py in forward-error units, the allowed ratios = 8 x
the model's worst), the oracle within a unit of 50-digit mpmath, every unit unchanged under a shift of the input, every mutant
of the model refused where the record says, the stop cases' margins, and the special configurations shown to be what they claim.

Figures of the long-double oracle alone are compared with the record to 1e-9; a ratio of the float64 model is compared within a
factor of two, as tests/test_tsne_hp_cpu.py does: numpy's einsum and sums differ in the last bit between builds and processors,
and a worst ratio is the maximum of that noise.  The allowed ratios are 8 x the RECORDED worst, exactly."""
import functools

import numpy as np
import pytest

import mds_hp_cases as K
import mds_oracle as MO
import mds_oracle_hp as HP

G = K.golden()
ALLOWED = G["allowed"]
DELTA = G["delta"]


def _within_two(a, b):
    return b / 2 <= a <= b * 2 or (a == b == 0.0)


@functools.lru_cache(maxsize=1)
def _measured():
    return K.measure()


def test_case_list_holds_the_shapes_it_is_for():
    assert set(G["dissimilarities"]) == set(K.DIS_BY_ID) and set(G["steps"]) == set(K.STEP_BY_ID)
    assert set(G["stops"]) == set(K.STOP_BY_ID) and set(G["mutants"]) == set(K.MUTANTS)
    shapes = {(c.n, c.f) for c in K.DIS}
    assert shapes == {(n, 9) for n in (2, 63, 64, 65, 129)} | {(65, f) for f in (1, 15, 16, 17, 33, 2772)}
    for s in shapes:
        assert {c.kind for c in K.DIS if (c.n, c.f) == s} == {"plain", "offset", "dups", "close"}
    both = {(n, d) for d in (1, 2, 4, 5, 16, 17, 64) for n in (9, 257)} | {
        (n, d) for d in (2, 5, 17) for n in (2, 7, 8, 9, 255, 256, 257, 513)}
    for kind in ("plain", "settled"):
        assert {(c.n, c.d) for c in K.STEPS if c.kind == kind} == both
    for kind in ("offset", "pairs", "collapsed"):
        assert {(c.n, c.d) for c in K.STEPS if c.kind == kind} == {s for s in both if s[1] in (2, 5, 17)}
    blocks = lambda c: -(-c.n // (8 if c.d <= 4 else 2 if c.d <= 16 else 1))      # noqa: E731
    assert [(c.n, c.d, blocks(c)) for c in K.REDUCTIONS] == [(2048, 2, 256), (2049, 2, 257), (512, 5, 256), (513, 5, 257),
                                                            (256, 17, 256), (257, 17, 257)]
    assert all(c.rows == sorted({0, 255, 256, c.n - 2, c.n - 1} - {c.n}) for c in K.REDUCTIONS)
    assert {(c.n, c.d, c.T) for c in K.STOPS} == {(n, d, T) for n, d in ((65, 2), (257, 5)) for T in (1, 2, 3)}
    assert max(c.n for c in K.STEPS + K.REDUCTIONS + K.STOPS) == 2049


def test_inputs_are_the_recorded_ones():
    for c in K.DIS:
        assert K.sha(c.X()) == G["dissimilarities"][c.id]["X"], c.id
    for c in K.STEPS + K.REDUCTIONS:
        g = G["steps"][c.id]
        assert [K.sha(a) for a in (c.X(), c.D0(), c.Y())] == [g[k] for k in ("X", "D", "Y")], c.id
    for c in K.STOPS:
        g = G["stops"][c.id]
        assert [K.sha(a) for a in (c.X(), c.D0(), c.Y0())] == [g[k] for k in ("X", "D", "Y0")] and c.seed == g["seed"], c.id


def test_allowed_ratios_are_eight_times_the_models_worst():
    """The model passes the comparison the GPU test uses on every case, each recorded ratio is at most allowed / 8 and the
    recomputed one within a factor of two of it; the allowed ratio is 8 x the recorded worst of the named case."""
    m = _measured()
    assert G["factor"] == K.FACTOR == 8 and G["quantities"] == list(K.QUANTITIES) and G["unit_eps"] == 2.0 ** -52
    per = {q: {} for q in K.QUANTITIES}
    for sec, keys in (("dissimilarities", {"D": "ratio"}), ("steps", {"Y1": "Y1", "stress": "stress"}), ("stops", {"v": "v", "Y1": "Y1"})):
        for cid, g in G[sec].items():
            for q, k in keys.items():
                rec = g["ratio"] if sec == "dissimilarities" else g["ratios"][k]
                got = m[sec][cid]["ratio"] if sec == "dissimilarities" else m[sec][cid]["ratios"][k]
                per[q][cid] = rec
                assert rec <= ALLOWED[q] / K.FACTOR and got <= ALLOWED[q], (cid, q, rec, got)
                if rec > ALLOWED[q] / 64:         # (a ratio far below the worst is a few roundings: its noise is of its own size)
                    assert _within_two(got, rec), (cid, q, got, rec)
    for q in K.QUANTITIES:
        w = G["worst"][q]
        assert w["ratio"] == max(per[q].values()) == per[q][w["case"]] and ALLOWED[q] == 8 * w["ratio"] and 0 < ALLOWED[q] < 1e3
        assert _within_two(m["worst"][q]["ratio"], w["ratio"]), (q, m["worst"][q], w)
    assert DELTA == ALLOWED["v"] * 2.0 ** -52
    print("worst |model - oracle| / unit: %s; allowed %s" % ({q: m["worst"][q] for q in K.QUANTITIES}, ALLOWED))


def test_oracle_is_within_a_unit_of_mpmath():
    pytest.importorskip("mpmath")
    rec = G["oracle_vs_mpmath"]
    assert set(rec) == {"D_n12_f3", "step_n12_d2", "settled_n12_d2"}
    got = K.mp_distances()
    print("|oracle - mpmath| / unit: %s" % got)
    for cid, d in got.items():
        assert set(d) == set(rec[cid])
        for k, v in d.items():
            assert v <= 2.0 ** -11 and v == pytest.approx(rec[cid][k], rel=1e-3, abs=1e-12), (cid, k, v)
            if k in ALLOWED:
                assert 1000 * v <= ALLOWED[k], (cid, k)


def _grid(a):
    """a rounded to multiples of 2^-30, so that a + 2^13 is exact in float64 and every difference is unchanged."""
    return np.round(a * 2.0 ** 30) / 2.0 ** 30


def test_every_unit_is_unchanged_under_a_shift_of_the_input():
    shift = 2.0 ** 13
    X = _grid(K.blobs(65, 17, 5))
    X[3] = X[2]
    (D, uD), (Ds, uDs) = HP.dissimilarities(X), HP.dissimilarities(X + shift)
    assert ((X + shift) - shift == X).all() and np.array_equal(D, Ds) and np.array_equal(uD, uDs) and (uD > 0).sum() == 65 * 64 - 2
    D64 = D.astype(np.float64)
    for d in (2, 5, 17):
        Y = _grid(np.random.RandomState(d).uniform(size=(65, d)))
        Y[1] = Y[0]
        a, b = HP.step(Y, D64), HP.step(Y + shift, D64)
        for k in ("Y1", "u_Y1", "stress", "u_stress", "sumsq", "u_sumsq"):
            assert np.array_equal(a[k], b[k]), (d, k)
        assert (a["u_Y1"] > 0).all() and a["u_stress"] > 0 and a["u_sumsq"] > 0
        ra, rb = HP.run(Y, D64, 3, 0.0), HP.run(Y + shift, D64, 3, 0.0)
        assert all(np.array_equal(p, q) for p, q in zip(ra["u_states"], rb["u_states"])) and len(ra["u_states"]) == 3
    # and against the norm of the input: the unit of a far configuration is that of the near one
    Y = K.StepCase(257, 5, "plain").Y()
    near, far = HP.step(Y, K.StepCase(257, 5).D0()), HP.step(Y + 1e4, K.StepCase(257, 5).D0())
    assert np.all(far["u_Y1"] <= near["u_Y1"] * 1.001) and far["u_stress"] <= near["u_stress"] * 1.001


def test_oracle_sums_are_serial():
    """1 followed by 1999 terms of 3e-20 (each below half an ulp of 1 in long double): a serial sum stays at exactly 1, a
    pairwise or tiled one gathers the small terms first and does not."""
    row = np.full(2000, 3e-20, dtype=HP.LD)
    row[0] = 1
    assert HP._rowsum(np.vstack([row, row]))[1] == 1 and HP._sum(row) == 1 and HP._rowsum(row[None, :])[0] == 1
    assert np.add.reduce(row) != 1          # (numpy's own sum along a contiguous axis is the pairwise one)


def test_oracle_run_follows_sklearns_loop():
    """n_iter and the trace of the oracle's run on a small case against the float64 driver, which tests/test_mds_cpu.py holds
    to sklearn's recorded n_iter: the same passes, the same stop."""
    c = K.STOPS[0]
    for max_iter, eps in ((1, 0.0), (2, 1e300), (5, 0.0), (5, 0.06), (5, 0.085)):
        o = HP.run(c.Y0(), c.D0(), max_iter, eps)
        Y, s, it, trace, vs = K.model_run(c.Y0(), c.D0(), max_iter, eps)
        assert o["n_iter"] == it == len(o["trace"]) == len(o["states"]) == len(trace), (max_iter, eps)
        assert float(o["trace"][-1]) == pytest.approx(s, rel=1e-12) and np.allclose(o["states"][-1].astype(np.float64), Y, rtol=0, atol=1e-12)
    assert [HP.run(c.Y0(), c.D0(), 5, e)["n_iter"] for e in (0.06, 0.085)] == [4, 3]


def test_every_mutant_fails_where_the_record_says():
    m = _measured()
    for name, (what, sites) in K.MUTANTS.items():
        rec = G["mutants"][name]
        assert rec["what"] == what and [(f["case"], f["quantity"]) for f in rec["fails"]] == [(s[0], s[1]) for s in sites]
        for f, g in zip(rec["fails"], m["mutants"][name]["fails"]):
            q = f["quantity"]
            print("%s on %s: %s at %.3g x unit, allowed %.3g" % (name, f["case"], q, g["ratio"], ALLOWED[q]))
            assert f["over_allowed"] == f["ratio"] / ALLOWED[q] > 8 and g["ratio"] > 8 * ALLOWED[q], (name, f, g)
            assert _within_two(g["ratio"], f["ratio"]), (name, f, g)
    # the model passes on those very cases (test_allowed_ratios...), and Gram forms pass where there is no offset: it is the
    # offset and the close pairs that convict them
    assert K._step_ratio("plain/n9_d17", "Y1", step=K.gram_step) < 1e-3 * K._step_ratio("offset/n9_d17", "Y1", step=K.gram_step)


def test_stop_cases_hold_their_margins_and_convict_the_wrong_denominator():
    runner = lambda sums: (lambda Y0, mi, eps: K.model_run(Y0, c.D0(), mi, eps, sums=sums)[:4])      # noqa: E731
    for c in K.STOPS:
        g, o = G["stops"][c.id], K.oracle_run(c)
        assert [float(v) for v in o["v"][1:]] == pytest.approx(g["v"], rel=1e-9) and len(g["v"]) == K.STOP_ITERS - 1
        assert g["fall"] > 0.02 and 1 - float(o["trace"][c.T] / o["trace"][c.T - 1]) == pytest.approx(g["fall"], rel=1e-9)
        if c.T > 1:
            assert K.margin(o["v"], c.T) == pytest.approx(g["margin"], rel=1e-9) and g["margin"] > 0.05 > 1e6 * DELTA
        else:
            assert g["margin"] is None
        r = K.check_stop(c, o, DELTA, runner(MO.stress), ALLOWED["Y1"], what="float64 model")
        assert r <= ALLOWED["Y1"] / K.FACTOR
        with pytest.raises(AssertionError):
            K.check_stop(c, o, DELTA, runner(K.distD_sums), ALLOWED["Y1"], what="mutant")


def test_driver_edges_on_the_model():
    for n, d in K.DRIVER_SHAPES:
        D = K.StepCase(n, d).D0()
        K.check_driver(n, d, D, lambda Y0, mi, eps: K.model_run(Y0, D, mi, eps)[:4], ALLOWED, what="float64 model")


def test_collapsed_and_pairs_have_the_zero_structure_they_promise():
    for c in K.STEPS:
        Y, D = c.Y(), c.D0()
        dist = MO.distances(Y)
        off = ~np.eye(c.n, dtype=bool)
        if c.kind == "collapsed":
            assert (Y == Y[0]).all() and (D[off] > 0).all()
            o = HP.step(Y, D)
            assert not o["Y1"].any() and not o["u_Y1"].any() and o["sumsq"] == 0
            half = HP._sum(HP._rowsum(HP._ld(D) ** 2)) / 2
            assert abs(o["stress"] - half) <= o["u_stress"] and 0 < o["u_stress"] < 1e-14 * half
        elif c.kind == "pairs":
            assert dist[0, 1] == 0 and (Y[0] == Y[1]).all()
            if c.n >= 4:
                assert D[0, 1] == 0 and dist[2, 3] == 0 and D[2, 3] > 0
            else:
                assert D[0, 1] > 0
            if c.n >= 6:
                assert 0 < dist[4, 5] < MO.ZERO_DIST and D[4, 5] > 0
                assert (dist[off] == 0).sum() == 4 and (D[off] == 0).sum() == 2
        else:
            assert (dist[off] > 0).all() and (D[off] > 0).all(), c.id
        if c.kind == "offset":
            assert Y.min() >= 1e4
        if c.kind == "settled":           # (a line, d = 1, cannot hold three blobs: there the stress only has to have fallen)
            s, s0 = MO.stress(Y, D)[0], MO.stress(K.StepCase(c.n, c.d).Y(), D)[0]
            assert s < (1e-3 * (D * D).sum() / 2 if c.d > 1 else 0.75 * s0), c.id
    for c in K.DIS:
        o = HP.dissimilarities(c.X())[0]
        q = max(1, c.n // 4)
        zeros = int((o == 0).sum()) - c.n
        assert zeros == G["dissimilarities"][c.id]["zeros"] - c.n == (2 * q if c.kind == "dups" else 0), c.id
        if c.kind == "close":
            near = o[np.arange(q), c.n - q + np.arange(q)]
            assert (near > 0).all() and (near < 1e-8 * np.sqrt(c.f)).all() and np.abs(c.X()).max() < 2
        if c.kind == "offset":
            assert c.X().min() >= 1e4
