"""The extended-precision t-SNE pin without a GPU: tests/golden/tsne_hp.json re-derived (input hashes, bisection margins, the
float64 model of tests/tsne_oracle.py against the long-double oracle of tests/tsne_oracle_hp.py in forward-error units, the allowed
ratios = 8 x the model's worst), the discontinuities shown to be decided, the undecided gains bounded, the clamp and offset cases
shown to be what they are for, two recorded rows recomputed, and the oracle's distance from 50-digit mpmath."""
import functools
import os

import numpy as np
import pytest

import tsne_hp_cases as K
import tsne_oracle as TO
import tsne_oracle_hp as HP

G = K.golden()
ALLOWED = G["allowed"]


def _near(a, b):
    """A re-derived long-double figure against its record."""
    return a == pytest.approx(b, rel=1e-3, abs=1e-300)


def _within_two(a, b):
    """A figure of the float64 model against its record: numpy's exp, log and BLAS differ in the last bit between builds and
    processors, and a worst ratio is the maximum of that noise."""
    return b / 2 <= a <= b * 2


@functools.lru_cache(maxsize=1)
def _measured():
    """({affinity case: (m_tol, m_sign, tries == 50, q ratio)}, {step case: (ratios, undecided, Q_clamped, oracle gains)})"""
    aff, steps = {}, {}
    for c in K.AFF:
        o = K.oracle_aff(c)
        beta, tries, q = TO.affinities(c.X(), c.perplexity)
        K.check_aff(c, o, beta, tries, q, ALLOWED["q"], what="float64 model")
        aff[c.id] = K.margins(c, o) + (int((o["tries"] == 50).sum()), HP.ratio(q, o["q"], o["u_q"]))
    for c in K.STEPS:
        r, st, m = K.model_step(c)
        if not c.recorded:
            assert K.margins(c.aff(), K.step_aff(c))[0] > K.MARGIN and K.margins(c.aff(), K.step_aff(c))[1] > K.MARGIN, c.id
        r.update(K.check_step(c, st, m.Y, m.iY, m.gains, [] if m.cost is None else [m.cost], ALLOWED, what="float64 model"))
        steps[c.id] = (r, int(K.undecided(st, ALLOWED["dY"]).sum()), st["Q_clamped"], st["gains"])
    return aff, steps


def test_case_list_holds_the_shapes_it_is_for():
    assert set(G["affinity"]) == set(K.AFF_BY_ID) and set(G["steps"]) == set(K.STEP_BY_ID)
    assert set(G["recorded"]) == set(K.RECORDED)
    plain = {(c.n, c.f) for c in K.AFF if c.kind == "plain"}
    assert {(n, 5) for n in (2, 3, 63, 64, 65, 1023, 1024, 1025)} | {(n, f) for n in (65, 1025) for f in (1, 5, 64)} <= plain
    assert {(c.kind, c.n) for c in K.AFF if c.kind != "plain"} == {("offset", 65), ("cap_up", 65), ("cap_down", 2), ("cap_down", 65)}
    assert {K.RECORDED[r][:2] for r in ("n8192_f5", "n8193_f5")} == {(8192, 5), (8193, 5)}
    steps = {(c.n, c.d) for c in K.STEPS}
    assert {(67, d) for d in (1, 2, 4, 5, 16, 17, 64)} | {(n, 2) for n in (7, 8, 9, 15, 16, 17)} <= steps
    assert {(n, 5) for n in (2, 3, 256, 257)} | {(n, d) for n in (255, 256, 257) for d in (2, 5, 17)} <= steps
    assert {(257, 17), (513, 5), (2049, 2), (512, 5)} <= steps
    for d in (2, 5, 17):            # one shape per instantiation through every phase switch and both kinds of iteration
        assert {c.t for c in K.STEPS if (c.n, c.d, c.kind) == (65, d, "plain")} == {0, 9, 19, 20, 99, 100, 101, 109}
    # more than 256 partials on a cost iteration too (tsne_sum over cpart), and exactly 256
    from_blocks = lambda c: -(-c.n // (8 if c.d <= 4 else 2 if c.d <= 16 else 1))      # noqa: E731
    assert {from_blocks(c) for c in K.STEPS if (c.t + 1) % 10 == 0} >= {256, 257}
    kinds = {(c.kind, (c.t + 1) % 10 == 0) for c in K.STEPS}
    assert {("far", False), ("far", True), ("coincident", True), ("min_gain", False)} <= kinds
    X = K.outlier_X()
    assert X.shape == (1025, 5) and (X[1024] == 1e200).all() and np.abs(X[:1024]).max() < 10
    assert K.CENTRE_N * K.CENTRE_D == 1024 * 256 + 64


def test_inputs_are_the_recorded_ones():
    for c in K.AFF:
        assert K.sha(c.X()) == G["affinity"][c.id]["X"] and c.seed == G["affinity"][c.id]["seed"]
    for c in K.STEPS:
        Y, iY, gains = c.state(K.step_aff(c)["q"])
        g = G["steps"][c.id]
        assert [K.sha(a) for a in (c.X(), Y, iY, gains)] == [g[k] for k in ("X", "Y", "iY", "gains")], c.id
        assert (iY == 0).any() or c.kind == "min_gain"
        assert (iY > 0).any() and (iY < 0).any()
    for rid, (n, f, seed) in K.RECORDED.items():
        g = G["recorded"][rid]
        assert K.sha(K.blobs(n, f, seed)) == g["X"]
        assert K.sha(np.load(os.path.join(K.DIR, rid + "_rows.npy"))) == g["rows_sha"]
        if "q_sha" in g:
            assert K.sha(np.load(os.path.join(K.DIR, rid + "_q.npy"))) == g["q_sha"]
            assert K.sha(np.load(os.path.join(K.DIR, rid + "_uq.npy"))) == g["uq_sha"]
            assert g["sampled_rows"] == K.SAMPLED_ROWS(n)
    X, Y0, _p = K.centre_inputs()
    assert (K.sha(X), K.sha(Y0)) == (G["centring"]["X"], G["centring"]["Y0"])
    sizes = [os.path.getsize(os.path.join(K.DIR, f)) for f in os.listdir(K.DIR)] + [os.path.getsize(K.JSON)]
    assert max(sizes) < 1e6 and sum(sizes) < 3e6


def test_every_compared_bisection_decision_is_decided():
    """Each uncapped row's margins exceed 1e-9; the cases meant to sit on the cap are listed and sit there."""
    aff, _steps = _measured()
    smallest = np.inf
    for c in K.AFF:
        m_tol, m_sign, capped, _r = aff[c.id]
        g = G["affinity"][c.id]
        assert g["cap"] == c.cap and capped == g["tries_50"] == {None: 0, "down": c.n, "up": K.DUPS}[c.cap], c.id
        assert m_tol > K.MARGIN and m_sign > K.MARGIN, (c.id, m_tol, m_sign)
        assert _near(m_tol, g["m_tol"]) and _near(m_sign, g["m_sign"]), c.id
        smallest = min(smallest, m_tol, m_sign)
    for rid in K.RECORDED:
        beta, tries, m_tol, m_sign = K.recorded_arrays(rid)
        g = G["recorded"][rid]
        assert (m_tol.min(), m_sign.min(), tries.max()) == (g["m_tol"], g["m_sign"], g["max_tries"]) and tries.max() < 50
        assert m_tol.min() > K.MARGIN and m_sign.min() > K.MARGIN
        smallest = min(smallest, m_tol.min(), m_sign.min())
    assert [c.id for c in K.AFF if c.cap] == ["plain/n2_f5", "cap_up/n65_f5", "cap_down/n2_f5", "cap_down/n65_f5"]
    print("smallest decision margin over all compared rows: %.3g (required %.3g)" % (smallest, K.MARGIN))


def test_allowed_ratios_are_eight_times_the_models_worst():
    """Every case of the model passes the comparison the GPU test uses (in _measured); the worst ratio per quantity is within a
    factor of two of the record, and the allowed ratio is 8 x the recorded worst."""
    aff, steps = _measured()
    assert G["factor"] == K.FACTOR == 8 and G["quantities"] == list(K.QUANTITIES) and G["unit_eps"] == 2.0 ** -52
    worst = dict.fromkeys(K.QUANTITIES, 0.0)
    for cid, v in aff.items():
        worst["q"] = max(worst["q"], v[3])
    for cid, (r, _u, _c, _g) in steps.items():
        for k in K.QUANTITIES:
            if k in r:
                worst[k] = max(worst[k], r[k])
    print("worst |model - oracle| / unit: %s; allowed %s" % (worst, ALLOWED))
    for k in K.QUANTITIES:
        rec = max([v["ratios"].get(k, 0.0) for v in G["steps"].values()]
                  + ([v["q"] for v in G["affinity"].values()] if k == "q" else []))
        assert G["worst"][k] == rec and ALLOWED[k] == 8 * rec and 0 < ALLOWED[k] < 1e3
        assert _within_two(worst[k], rec), (k, worst[k], rec)


def test_gram_form_on_the_offset_case_exceeds_the_allowed_ratio():
    """X + 1e4: the same differences, norms of 1e8.  The model (direct differences) stays within the allowed ratio (above); the
    reference's Gram form in float64, from the same betas, does not: the unit would catch a kernel that had moved to it."""
    c = K.AFF_BY_ID["offset/n65_f5"]
    o = K.oracle_aff(c)
    assert c.seed == K.AFF_BY_ID["plain/n65_f5"].seed and np.abs(c.X()).min() > 9990
    r = HP.ratio(K.gram_q(c.X(), o["beta"]), o["q"], o["u_q"])
    print("Gram-form q on %s: %.3g x unit (allowed %.3g)" % (c.id, r, ALLOWED["q"]))
    assert r > 1000 * ALLOWED["q"] and _within_two(r, G["gram_on_offset"]["q"])


def test_undecided_gains_are_bounded_and_the_special_states_are_what_they_claim():
    _aff, steps = _measured()
    for c in K.STEPS:
        r, und, clamped, gains = steps[c.id]
        g = G["steps"][c.id]
        assert und <= K.skip_cap(c.n * c.d) and und == g["undecided"] and g["entries"] == c.n * c.d, (c.id, und)
        assert r["skipped"] <= und
        if c.kind == "far":
            assert clamped > 0.25 and _near(clamped, g["Q_clamped"]), (c.id, clamped)
        elif c.kind != "coincident" and c.n > 3:
            assert clamped == 0.0, c.id
        if c.kind == "min_gain":            # 0.0124 x 0.8 < 0.01 is clamped, 0.0126 x 0.8 is not; n d is odd: both occur
            assert set(np.unique(gains).tolist()) == {0.01, 0.0126 * 0.8} and 0.0124 * 0.8 < 0.01 < 0.0126 * 0.8
        if c.kind == "coincident":
            Y = c.state()[0]
            assert (Y[1:4] == Y[0]).all() and (Y[6] == Y[5]).all()


def test_oracle_sums_are_serial():
    """1 followed by 1999 terms of 3e-20 (each below half an ulp of 1 in long double): a serial sum stays at exactly 1, a
    pairwise or tiled one gathers the small terms first and does not."""
    row = np.full(2000, 3e-20, dtype=HP.LD)
    row[0] = 1
    assert HP._rowsum(np.vstack([row, row]))[1] == 1 and HP._sum(row) == 1 and HP._rowsum(row[None, :])[0] == 1
    assert np.add.reduce(row) != 1          # (numpy's own sum along a contiguous axis is the pairwise one)


def test_two_recorded_rows_of_n8193_are_the_oracles():
    """Rows 1024 and n - 1 of the record, every column, recomputed from the recorded betas."""
    rid = "n8193_f5"
    n, f, seed = K.RECORDED[rid]
    g = G["recorded"][rid]
    beta = K.recorded_arrays(rid)[0]
    rows = K.SAMPLED_ROWS(n)
    pick = [2, 5]
    cols = np.arange(n)
    o = HP.affinities(K.blobs(n, f, seed), beta=beta, total=K.ld(g["total"]), rel_total=K.ld(g["rel_total"]),
                      rows=[rows[k] for k in pick], cols=cols)
    q = np.load(os.path.join(K.DIR, rid + "_q.npy"))[pick][:, cols]
    uq = np.load(os.path.join(K.DIR, rid + "_uq.npy"))[pick][:, cols]
    assert np.array_equal(o["q"].astype(np.float64), q)
    assert np.all(uq >= o["u_q"]) and np.all(uq <= o["u_q"] * (1 + 1e-5) + np.abs(q - o["q"]) * 1.001)


def test_centring_case_record():
    """S of the centring case against a float64 evaluation (Gram form through BLAS: norms of 1e5 against distances of 30)."""
    g = G["centring"]
    _X, Y0, perplexity = K.centre_inputs()
    assert perplexity > K.CENTRE_N - 1 and g["rows"] == K.CENTRE_ROWS
    assert np.all(np.abs(Y0.mean(axis=0) - np.arange(K.CENTRE_D)) < 0.1)
    s = (Y0 * Y0).sum(axis=1)
    num = 1.0 / (1.0 + np.maximum(s[:, None] + s[None, :] - 2.0 * (Y0 @ Y0.T), 0.0))
    np.fill_diagonal(num, 0.0)
    assert abs(num.sum() - float(K.ld(g["S"]))) <= 1e-9 * num.sum()
    assert 0 < float(K.ld(g["rel_S"])) < 1e3 * 2.0 ** -52
    assert float(K.centre_q()) > 1e4 * float(HP.Q_FLOOR)
    assert g["model_ratio"] == K.centre_model() > 0 and g["allowed"] == K.FACTOR * g["model_ratio"]


def test_oracle_is_far_closer_to_mpmath_than_the_allowed_ratios():
    pytest.importorskip("mpmath")
    rec = G["oracle_vs_mpmath"]
    assert set(rec) == {"affinities_n12_f3", "step_n12_d2_t0", "step_n12_d2_t109"} and "cost" in rec["step_n12_d2_t109"]
    got = K.mp_distances()
    print("|oracle - mpmath| / unit: %s" % got)
    for cid, d in got.items():
        assert set(d) == set(rec[cid])
        for k, v in d.items():
            assert v <= 2.0 ** -11 and v == pytest.approx(rec[cid][k], rel=1e-3, abs=1e-12) and 1000 * v <= ALLOWED[k], (cid, k)
