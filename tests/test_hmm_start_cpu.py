"""The HMM's deterministic start and first EM rounds without a GPU: the inputs of tests/hmm_start_cases.py and the conditions they
must meet, the long-double oracle qualified against mpmath, the arithmetic of tests/golden/hmm_start.json, the float64 models of both
layouts against the oracle (the host one bit for bit against the library) - clean and with every seeded defect, which the
comparison routines of the GPU test must reject -, and the host-native fit of 0, 1 and 3 rounds against the oracle on every case."""
import os
import re

import numpy as np
import pytest

import hmm_estep_cases as E
import hmm_gpu_cases as H
import hmm_start_cases as S
import hmm_start_model as SM

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G = S.golden()
TOL = G["tolerance"]


# ---------------------------------------------------------------------------------------------------------- layouts and inputs
def test_sizes_bracket_every_change_of_both_layouts():
    kernels = open(os.path.join(REPO, "frisk_amd", "csrc", "hmm_kernels.h")).read()
    host = open(os.path.join(REPO, "frisk_amd", "csrc", "hmm_host.h")).read()
    assert re.search(r"constexpr int PARTS = %d;" % SM.PARTS, kernels) and re.search(r"constexpr int RED_T = %d;" % SM.RED_T, kernels)
    assert "std::min<int64_t>(PARTS, std::max<int64_t>(1, n / RED_T))" in kernels
    assert re.search(r"constexpr int PIECES = %d;" % SM.HOST_PIECES, host)
    assert "std::min<int64_t>(PIECES, std::max<int64_t>(1, n / %d))" % SM.HOST_MIN in host
    assert "std::min<int64_t>(PIECES, std::max<int64_t>(1, n / %d))" % SM.HOST_MIN_E in host
    assert [SM.parts_of(n) for n in (511, 512, 767, 768, 262143, 262144, 262145)] == [1, 2, 2, 3, 1023, 1024, 1024]
    assert set(np.diff(SM.bounds(262144 + 1023, SM.PARTS)).tolist()) == {256, 257}
    assert [SM.host_parts_of(n) for n in (8191, 8192, 1048575, 1048576, 1048577)] == [1, 2, 255, 256, 256]
    assert set(S.DEVICE_SIZES) | set(S.HOST_SIZES) == set(S.SIZES) and len(S.SIZES) == 24
    assert set(S.ROUND_SIZES) == set(E.SMALL) | set(E.LARGE)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_start_inputs_regenerate_and_meet_the_conditions(family):
    """Every size regenerates to its recorded sha256; up to 8193 windows the oracle's account is recomputed here and held to the
    conditions (the larger ones were, when the file was made: the generator stops on a case that fails one)."""
    for n in S.SIZES:
        x = S.start_input(family, n)
        assert x.shape == (n,) and np.all(np.isfinite(x))
        assert H.sha(x) == G["start_cases"][S.start_id(family, n)]["sha256"], (family, n)
    for n in S.SMALL:
        st = S.start_account(family, n)
        S.start_conditions(family, n, st)
        assert st["rounds"] == G["start_cases"][S.start_id(family, n)]["rounds"]
    rounds = [G["start_cases"][S.start_id(family, n)]["rounds"] for n in S.SIZES]
    print(family, "rounds of 2-means:", dict(zip(S.SIZES, rounds)))
    if family == "overlap":
        assert all(r >= S.SLOW_ROUNDS for n, r in zip(S.SIZES, rounds) if n >= S.SLOW_FROM)
    if family.startswith("edges"):
        for n in S.SIZES[1:]:
            x = S.start_input(family, n)
            pmin, pmax = S.edge_positions(int(family[5:]), n)
            assert int(np.argmin(x)) == pmin and int(np.argmax(x)) == pmax and np.sum(x == x.min()) == 1 and np.sum(x == x.max()) == 1
            # round 1 meets the stop rule: the start's means are the two extremes themselves, whatever else the input holds
            ref = S.start_reference(family, n)
            assert ref["rounds"] == 1 and [float(v) for v in ref["means"]] == [S.EDGE_MIN, S.EDGE_MAX]
    if family == "ties":
        for n in S.SIZES:
            x = S.start_input(family, n)
            assert np.array_equal(x * 1024, np.round(x * 1024))            # dyadic: every sum is exact
            if n >= 8:
                assert x.min() == 0.0 and x.max() == 1.0 and np.all(x[S.tie_positions(n)] == 0.5) and len(S.tie_positions(n)) >= 4
                assert np.sum(x[x != 0.5]) * 2 == np.sum(x != 0.5)          # mirror images: the others average 1 / 2 exactly
        assert all(S.start_account("ties", n)["ties"][0] >= 4 for n in S.SMALL if n >= 8)


def test_edge_families_reach_the_chunk_bounds_they_are_for():
    n = 262144 + 1023
    D, Hc = SM.bounds(n, SM.parts_of(n)), SM.bounds(1048577, SM.host_parts_of(1048577))
    assert S.edge_positions(0, n) == (0, n - 1) and S.edge_positions(1, n) == (n - 1, 0)
    assert S.edge_positions(2, n) == (int(D[512]) - 1, int(D[512])) and S.edge_positions(3, 1048577) == (int(Hc[128]), int(Hc[128]) - 1)
    assert S.edge_positions(4, n) == (int(D[1023]) + 255, int(D[1023]) + 256) and n - int(D[1023]) == 257      # thread 255, then thread 0 again
    assert S.edge_positions(5, n) == (256, 255)
    assert S.edge_positions(4, 2) == (0, 1) and S.edge_positions(5, 2) == (0, 1) and S.edge_positions(4, 256) == (254, 255)


@pytest.mark.parametrize("family", S.ROUND_FAMILIES)
def test_round_inputs_regenerate_and_keep_their_gains_away_from_tol(family):
    for n in S.ROUND_SIZES:
        assert H.sha(S.round_input(family, n)) == G["round_cases"][S.round_id(family, n)]["sha256"], (family, n)
    for n in E.SMALL:
        S.round_conditions(family, n, S.round_reference(family, n)["lls"])


def test_the_hundred_round_cap_is_not_reached_and_not_claimed():
    """No input here of at most 4096 windows - nor any other - needs more than a third of the 100 rounds 2-means may take: the cap
    itself stays unpinned (DESIGN.md says so)."""
    most = max(c["rounds"] for c in G["start_cases"].values())
    assert G["max_rounds_up_to_4096"] == max(c["rounds"] for c in G["start_cases"].values() if c["n"] <= 4096)
    assert S.SLOW_ROUNDS <= G["max_rounds_up_to_4096"] <= most < 100


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("family", S.FAMILIES)
def test_start_oracle_is_sixteen_times_closer_to_mpmath_than_the_tolerance(family):
    import hmm_oracle_hp as O
    for n in (1, 2, 255, 256, 257):
        d = dict(zip(S.START_Q, O.start_distance_from_mp(S.start_input(family, n), S.MIN_COVAR)))
        print("%s: oracle against mpmath %s" % (S.start_id(family, n), d))
        for q in S.START_Q:
            assert d[q] <= max(G["oracle_vs_mpmath"][q], 1e-19) and S.ORACLE_MARGIN * d[q] <= TOL[q]


@pytest.mark.parametrize("family", S.ROUND_FAMILIES)
def test_round_oracle_is_sixteen_times_closer_to_mpmath_than_the_tolerance(family):
    import hmm_oracle_hp as O
    for n in (1, 2, 33, 64, 129):
        d = O.rounds_distance_from_mp(S.round_input(family, n), S.ROUNDS, S.MIN_COVAR, S.COVARS_PRIOR)
        d = {"fit%d_%s" % (r, k): d[r][i] for r in S.ROUNDS for i, k in enumerate(("params", "loglik"))}
        print("%s: oracle against mpmath %s" % (S.round_id(family, n), d))
        for q in S.ROUND_Q:
            assert d[q] <= max(G["oracle_vs_mpmath"][q], 1e-19) and S.ORACLE_MARGIN * d[q] <= TOL[q]


def test_long_doubles_survive_the_file():
    v = np.longdouble(1) / np.longdouble(3) * np.longdouble(1000)
    assert S.join(S.split(v)) == v and S.join(S.split(-v)) == -v and S.join(S.split(np.longdouble(0.1))) == np.longdouble(0.1)


def test_tolerance_file_is_the_stated_multiple_of_the_cpu_errors():
    assert G["factor"] == S.FACTOR == H.FACTOR == 8 and G["oracle_margin"] == S.ORACLE_MARGIN == 16
    assert G["margin"] == H.MARGIN == 1e-9 and G["stop_margin"] == S.STOP_MARGIN == 1e-3 and G["gap"] == H.GAP
    assert G["sizes"] == list(S.SIZES) and G["large"] == list(S.LARGE) and G["round_sizes"] == list(S.ROUND_SIZES)
    assert set(G["start_cases"]) == {S.start_id(*c) for c in S.start_cases()} and len(G["start_cases"]) == 13 * 24
    assert set(G["round_cases"]) == {S.round_id(*c) for c in S.round_cases()} and len(G["round_cases"]) == 3 * 22
    cases_of = lambda q: G["start_cases" if q in S.START_Q else "round_cases"].values()      # noqa: E731
    assert set(G["tolerance"]) == set(S.QUANTITIES) and set(G["error"]) == set(S.FORMS)
    for q in S.QUANTITIES:
        for f in S.FORMS:
            assert G["error"][f][q] == max(c["error"][f][q] for c in cases_of(q))      # every case counted: none exempted
        assert TOL[q] == 8 * max(G["error"][f][q] for f in S.FORMS)
        assert G["oracle_vs_mpmath"][q] == max(c["oracle_vs_mpmath"][q] for c in cases_of(q) if "oracle_vs_mpmath" in c)
        assert 16 * G["oracle_vs_mpmath"][q] <= TOL[q]
        assert 0 < TOL[q] < 1e-6              # (rounding, not a chosen number - and far below what a lost window changes)
        # the second bound of the round comparisons on the device: the two forms that work in scaled space, without the numpy
        # specification's log-space recursion
        tight = G["tolerance_scaled_forms"][q]
        assert tight == 8 * max(G["error"]["model"][q], G["error"]["host"][q]) and 16 * G["oracle_vs_mpmath"][q] <= tight <= TOL[q]
        assert tight < 1e-11
    assert all(("oracle" in c) == (c["n"] in S.LARGE) for c in G["start_cases"].values())
    assert all(("oracle" in c) == (c["n"] in E.LARGE) for c in G["round_cases"].values())
    assert all(("oracle_vs_mpmath" in c) == (c["n"] <= 257) for c in G["start_cases"].values())
    assert all(("oracle_vs_mpmath" in c) == (c["n"] <= 129) for c in G["round_cases"].values())
    assert os.path.getsize(S.JSON) < (1 << 20)
    print("errors", G["error"], "tolerance", TOL)


# ------------------------------------------------------------------------------------------------- the three forms, recomputed
@pytest.mark.parametrize("family", S.FAMILIES)
def test_start_errors_of_the_three_forms_recomputed_on_the_small_cases(family):
    """The numpy specification, the float64 model in the device's layout and the host-native library, up to 8193 windows: each
    within its recorded error (so within an eighth of the tolerance).  The model in the HOST's layout is the library bit for bit."""
    for n in S.SMALL:
        x = S.start_input(family, n)
        ref = S.start_reference(family, n)
        means, covar, rounds = SM.start(x, "device")
        assert rounds == ref["rounds"]
        got = {"model": (means, [covar, covar]), "numpy": S.fit_start(x, False)[1], "host": S.fit_start(x, True)[1]}
        for f in S.FORMS:
            e = S.start_errors(got[f], ref)
            assert all(e[q] <= G["error"][f][q] for q in S.START_Q), (f, family, n, e)
        hm, hc, hr = SM.start(x, "host")
        assert hr == ref["rounds"] and np.array_equal(got["host"][0], hm) and np.array_equal(got["host"][1], [hc, hc]), (family, n)


@pytest.mark.parametrize("family", S.ROUND_FAMILIES)
def test_round_errors_of_the_three_forms_recomputed_on_the_small_cases(family):
    for n in E.SMALL:
        x = S.round_input(family, n)
        ref = S.round_reference(family, n)
        model, spec = SM.fit(x, max(S.ROUNDS)), S.numpy_rounds(x)
        for r in S.ROUNDS:
            got = {"model": model[r - 1], "numpy": spec[r], "host": S.fit_rounds(x, r, True)[1]}
            for f in S.FORMS:
                e = S.round_errors(r, got[f], ref)
                assert all(e[q] <= G["error"][f][q] for q in e), (f, family, n, r, e)


# ----------------------------------------------------------------------------------------------------------------- the defects
def _rejected_start(layout, defect, cases):
    out = []
    for family, n in cases:
        means, covar, _r = SM.start(S.start_input(family, n), layout, defect)
        try:
            S.check_start(family, n, (means, [covar, covar]), what=defect)
        except AssertionError:
            out.append(S.start_id(family, n))
    return out


@pytest.mark.parametrize("defect", SM.DEFECTS)
def test_start_comparison_rejects_a_seeded_defect(defect):
    """Each defect seeded into the models of both layouts, compared by the routine the GPU test uses."""
    cap = defect == "chunk_count_one_short_at_cap"
    cases = [("regimes", n) for n in (262143, 262144, 262145, 262144 + 1023)] if cap else S.start_cases(S.SMALL)
    dev = _rejected_start("device", defect, cases)
    print("%s, device layout: rejected on %d of %d cases, e.g. %s" % (defect, len(dev), len(cases), dev[:6]))
    if cap:
        assert dev == [S.start_id("regimes", n) for n in (262144, 262145, 262144 + 1023)]      # (below the cap it is no defect)
        return
    assert dev
    if defect == "ties_to_centre_1":
        assert all(c.startswith("ties-") for c in dev) and len(dev) >= len(S.SMALL) - 2      # every size that can hold a tie
    if defect == "last_chunk_not_in_range":
        # wherever an extreme lies in the last of two or more chunks: by construction in edges0, edges1 and edges4 at every such size
        assert set(dev) >= {S.start_id(f, n) for f in ("edges0", "edges1", "edges4") for n in S.SMALL if SM.parts_of(n) >= 2}
        return                                  # (the host takes its range serially: no chunk to leave out)
    if defect == "new_centres_kept":
        # 2-means on a few thousand windows ends on a partition that no longer changes, where the new centres ARE the previous ones:
        # below the cap only `offset` (whose first round already meets the stop rule) shows it; from 262144 windows on every draw does
        big = _rejected_start("device", defect, [("regimes", 262144), ("overlap", 262145)])
        assert len(big) == 2 and any(c.startswith("offset-") for c in dev)
    if defect == "one_pass_variance":
        assert any(c.startswith("offset-") for c in dev)
    host = _rejected_start("host", defect, cases)
    print("%s, host layout: rejected on %d of %d cases, e.g. %s" % (defect, len(host), len(cases), host[:6]))
    assert host


@pytest.mark.parametrize("defect", SM.FIT_DEFECTS + ("chunk_last_window_dropped", "variance_about_centre_0"))
def test_round_comparison_rejects_a_seeded_defect(defect):
    """A defect of the M step - or of the start, one and three rounds later - against the round comparison of the GPU test."""
    rejected = []
    for family, n in S.round_cases(E.SMALL):
        got = SM.fit(S.round_input(family, n), max(S.ROUNDS), defect=defect)
        try:
            for r in S.ROUNDS:
                S.check_device_rounds(family, n, r, got[r - 1], what=defect)
        except AssertionError:
            rejected.append(S.round_id(family, n))
    print("%s: rejected on %d of %d cases, e.g. %s" % (defect, len(rejected), len(S.round_cases(E.SMALL)), rejected[:6]))
    assert rejected
    if defect == "covars_about_old_means":
        # the outliers of `regimes` and `cuts` hold state 1's mean still from 64 windows on: what moves the means is `plain`
        assert any(c.startswith("rounds-plain-") and int(c.split("-")[2]) > 33 for c in rejected)


# ------------------------------------------------------------------------------------------------------ the host-native library
def _is_a_start(m):
    assert m.n_iter_ == 0 and m.loglik_ == -np.inf and m.means_[0] <= m.means_[1] and m.covars_[0] == m.covars_[1]
    assert np.array_equal(m.startprob_, [0.5, 0.5]) and np.array_equal(m.transmat_, [[0.5, 0.5], [0.5, 0.5]])


@pytest.mark.parametrize("family", S.FAMILIES)
def test_host_start_against_the_oracle_on_every_case(family):
    for n in S.SIZES:
        x = S.start_input(family, n)
        m, got = S.fit_start(x, True)
        e, msg = S.check_start(family, n, got, what="host-native")
        assert all(e[q] <= G["error"]["host"][q] for q in S.START_Q), msg
        _is_a_start(m)
        again = S.fit_start(x, True)[1]
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


@pytest.mark.parametrize("family", S.ROUND_FAMILIES)
def test_host_rounds_against_the_oracle_on_every_case(family):
    for n in S.ROUND_SIZES:
        x = S.round_input(family, n)
        for r in S.ROUNDS:
            m, got = S.fit_rounds(x, r, True)
            e, msg = S.check_rounds(family, n, r, got, what="host-native")
            assert all(e[q] <= G["error"]["host"][q] for q in e), msg
            assert m.n_iter_ == r and m.means_[0] <= m.means_[1]
            assert S.fit_rounds(x, r, True)[1] == got


@pytest.mark.parametrize("native", [False, True])
def test_constant_and_two_valued_inputs_give_exact_starts(native):
    """All windows equal: both means that value and both variances min_covar, bit for bit; two distinct values: the means are the two."""
    for n in S.SIZES:
        m, (means, covars) = S.fit_start(S.start_input("constant", n), native)
        assert means.tolist() == [0.1, 0.1] and covars.tolist() == [S.MIN_COVAR, S.MIN_COVAR], (n, means, covars)
        m, (means, covars) = S.fit_start(S.start_input("two_values", n), native)
        assert means.tolist() == ([0.03, 0.15] if n > 1 else [0.03, 0.03]), (n, means)
    for layout in ("device", "host"):
        for n in S.SMALL:
            assert SM.start(S.start_input("constant", n), layout)[:2] == ([0.1, 0.1], S.MIN_COVAR)
