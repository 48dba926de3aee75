"""The E step of the 2-state HMM without a GPU: the extended-precision oracle qualified against mpmath, the arithmetic of
tests/golden/hmm_estep.json, the float64 model of the device's piece scheme against the oracle - clean and with each of six seeded
defects, which the comparison routine of the GPU test must reject -, the host-native frisk_hmm_estep against the oracle on every
case, and the hook being the code the fit runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hmm_estep_cases as E
import hmm_gpu_cases as H
import hmm_piece_model as PM
from frisk_amd.hmm import GaussianHMM2

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
G = E.golden()
TOL = G["tolerance"]
PAIRS = [(m, f) for m in E.MODELS for f in E.FAMILIES]


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("model", list(E.MODELS))
def test_oracle_is_sixteen_times_closer_to_mpmath_than_the_tolerance(model):
    """50-digit mpmath, unscaled, at n <= 200 (sizes with one, two and four device pieces), both families; the float64 rounding of
    the values the tests compare with is counted as the oracle's."""
    import hmm_oracle_hp as O
    rounding = {"posterior": 2.0 ** -54, "statistics": 2.0 ** -53, "loglik": 2.0 ** -53}
    for family in E.FAMILIES:
        for n in (1, 2, 33, 64, 129):
            x = E.case_input(model, family, n)
            d = dict(zip(E.QUANTITIES, O.distance_from_mp(x, E.MODELS[model])))
            rec = G["cases"][E.case_id(model, family, n)]["oracle_vs_mpmath"]
            print("%s: oracle against mpmath %s (recorded %s)" % (E.case_id(model, family, n), d, rec))
            for q in E.QUANTITIES:
                assert d[q] <= max(G["oracle_vs_mpmath"][q], 1e-19)
                assert E.ORACLE_MARGIN * (d[q] + rounding[q]) <= TOL[q]
            # the log-space form, a second opinion at this size
            lp, ls, lll = O.e_step_logspace(x, E.MODELS[model])
            E.check(model, family, n, (lp.astype(np.float64), ls.astype(np.float64), float(lll)), what="log-space long double")


def test_tolerance_file_is_the_stated_multiple_of_the_cpu_errors():
    assert G["factor"] == E.FACTOR == H.FACTOR == 8 and G["oracle_margin"] == E.ORACLE_MARGIN == 16
    assert G["models"] == E.MODELS and G["small"] == list(E.SMALL) and G["large"] == list(E.LARGE)
    assert set(G["cases"]) == {E.case_id(*c) for c in E.all_cases(E.SMALL + E.LARGE)}
    for who in ("piece_model", "host"):
        for q in E.QUANTITIES:
            assert G["error"][who][q] == max(c[who][q] for c in G["cases"].values())
    for q in E.QUANTITIES:
        assert TOL[q] == 8 * max(G["error"]["piece_model"][q], G["error"]["host"][q])
        assert G["oracle_vs_mpmath"][q] == max(c["oracle_vs_mpmath"][q] for c in G["cases"].values() if "oracle_vs_mpmath" in c)
        assert 16 * (G["oracle_vs_mpmath"][q] + G["float64_rounding_of_the_reference"][q]) <= TOL[q]
        assert 0 < TOL[q] < 1e-12             # (double rounding, not a chosen number: a looser file is a changed measurement)
    assert all(("oracle_vs_mpmath" in c) == (c["n"] <= 200) for c in G["cases"].values())
    z = np.load(E.NPZ)
    assert set(z.files) == {E.case_id(*c) + s for c in E.all_cases(E.LARGE) for s in ("/post", "/stats")}
    assert os.path.getsize(E.NPZ) < (1 << 20)
    for c in E.all_cases(E.LARGE):
        assert z[E.case_id(*c) + "/post"].shape == (E.sample_windows(c[2]).size, 2) and z[E.case_id(*c) + "/stats"].shape == (9,)


def test_sample_windows_straddle_the_first_and_last_cuts():
    for n in E.LARGE:
        w = set(E.sample_windows(n).tolist())
        cut = PM.bounds(n, PM.pieces_of(n))
        for p in list(range(1, 9)) + list(range(PM.pieces_of(n) - 8, PM.pieces_of(n))):
            assert {cut[p] + d for d in range(-4, 4)} <= w
        assert len(w) >= 512
    assert PM.pieces_of(524287) == 16383 and PM.pieces_of(524288) == 16384 == PM.pieces_of(524289) == PM.PIECES
    lens = set(np.diff(PM.bounds(524288 + 16383, PM.PIECES)).tolist())
    assert lens == {32, 33}
    assert PM.pieces_of(63) == 1 and PM.pieces_of(64) == 2


# ------------------------------------------------------------------------------------------- the piece model and its defects
def test_inputs_regenerate_and_reach_the_regimes_they_are_for():
    for c in E.all_cases(E.SMALL + E.LARGE):
        assert H.sha(E.case_input(*c)) == G["cases"][E.case_id(*c)]["sha256"], c
    # an emission that underflows to exactly 0 on both sides of a cut, in both orders, and the forward walk's flush below 1e-200
    import hmm_oracle_hp as O
    n = 2049
    x = E.case_input("apart", "cuts", n)
    b = O.emissions(x, E.MODELS["apart"])[0].astype(np.float64)
    c = PM.bounds(n, PM.pieces_of(n))[2]
    assert b[c - 2:c + 2].tolist() == [[0.0, 1.0], [1.0, 0.0], [0.0, 1.0], [1.0, 0.0]]
    assert E.MODELS["apart"]["trans"][0][1] ** 3 < 1e-200


@pytest.mark.parametrize("model,family", PAIRS)
def test_piece_model_in_the_device_layout_is_within_the_recorded_error(model, family):
    for n in E.SMALL:
        got = PM.e_step(E.case_input(model, family, n), E.MODELS[model])
        e, _t = E.errors(n, got, E.reference(model, family, n))
        assert all(e[q] <= G["error"]["piece_model"][q] for q in E.QUANTITIES), (n, e)
        E.structure(n, got)


@pytest.mark.parametrize("defect", PM.DEFECTS)
def test_comparison_rejects_a_seeded_defect(defect):
    rejected = []
    for model, family, n in E.all_cases(E.SMALL):
        if PM.pieces_of(n) < 2 and defect != "flush_drops_held":
            continue                            # (a defect of the cut logic cannot show on one piece)
        try:
            got = PM.e_step(E.case_input(model, family, n), E.MODELS[model], defect=defect)
            E.check(model, family, n, got, what=defect)
        except (AssertionError, ZeroDivisionError, ValueError):
            rejected.append(E.case_id(model, family, n))
    print("%s: rejected on %d cases, e.g. %s" % (defect, len(rejected), rejected[:4]))
    # (a forward vector forgets where it started within a piece unless the model is sticky: first_step_not_skipped shows on `sticky`
    # alone, which is what that model is in the case set for)
    assert rejected


# ------------------------------------------------------------------------------------------------------------ frisk_hmm_estep
def test_estep_symbols_are_declared_and_exported_and_check_their_arguments():
    import __graft_entry__ as g
    g.build_hip()
    from frisk_amd import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "frisk_hip.h")).read(), flags=re.S)
    table = {n: a for n, _r, a in _ffi.SYMBOLS}
    assert re.search(r"\bint\s+frisk_hmm_estep\s*\(\s*const\s+double\s*\*\s*x\b", text)
    assert re.search(r"\bint\s+frisk_hmm_estep_gpu\s*\(\s*int\s+device\b", text)
    assert table["frisk_hmm_estep_gpu"] == [C.c_int] + table["frisk_hmm_estep"]
    lib = _ffi.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    good = dict(x=np.array([0.1, 0.2, 0.3]), means=np.array([0.04, 0.13]), covars=np.array([2e-4, 1.5e-3]), start=np.array([0.6, 0.4]),
                trans=np.array([0.97, 0.03, 0.08, 0.92]))
    post, stats = np.zeros((3, 2)), np.zeros(9)

    def call(fn, n=3, **kw):
        a = dict(good, **kw)
        args = (p(a["x"]), n, p(a["means"]), p(a["covars"]), p(a["start"]), p(a["trans"]), p(post), p(stats))
        return lib.frisk_hmm_estep(*args) if fn == "host" else lib.frisk_hmm_estep_gpu(0, *args)
    assert call("host") == _ffi.OK and abs(stats[0] + stats[1] - 3) < 1e-14
    nan, inf = float("nan"), float("inf")
    bad = [dict(n=0), dict(n=-1), dict(x=np.array([0.1, nan, 0.3])), dict(x=np.array([0.1, 0.2, inf])), dict(means=np.array([nan, 0.1])),
           dict(covars=np.array([0.0, 1e-3])), dict(covars=np.array([1e-3, -1e-3])), dict(covars=np.array([1e-3, inf])),
           dict(start=np.array([1.5, -0.5])), dict(start=np.array([nan, 0.5])), dict(trans=np.array([1.0, 0.0, -1e-9, 1.0])),
           dict(trans=np.array([0.5, 0.5, 0.5, 1.0 + 1e-9])), dict(trans=np.array([0.5, nan, 0.5, 0.5]))]
    for kw in bad:
        # (the device form: before any device is touched - there is none here)
        assert call("host", **kw) == _ffi.E_ARG and call("gpu", **kw) == _ffi.E_ARG, kw
    with pytest.raises(ValueError):
        H.model_of(H.KLD_MODEL, True).e_step(np.array([0.1, nan]))


@pytest.mark.parametrize("model,family", PAIRS)
def test_host_estep_against_the_oracle(model, family):
    """frisk_hmm_estep on every case: window by window up to 2049, against the recorded oracle values from 4095 on."""
    for n in E.SMALL + E.LARGE:
        x = E.case_input(model, family, n)
        got = E.host_e_step(model, x)
        e, msg = E.check(model, family, n, got, what="host-native")
        assert all(e[q] <= G["error"]["host"][q] for q in E.QUANTITIES), msg
        E.structure(n, got)
        again = E.host_e_step(model, x)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("model", ["kld", "tinyvar"])
def test_numpy_estep_is_the_same_quantity(model):
    """native=False: _forward_backward and the fit's own xi expression (log space, so only to its accuracy)."""
    for family in E.FAMILIES:
        x = E.case_input(model, family, 129)
        post, stats, ll = E.host_e_step(model, x, native=False)
        _w, rp, rs, rll = E.reference(model, family, 129)
        assert np.max(np.abs(post - rp)) < 1e-9 and np.max(np.abs(stats - rs)) < 1e-9 * 129 and abs(ll - rll) < 1e-9 * abs(rll)


def m_step(x, post, stats, cov_sums, covars_prior=1e-2):
    """hmm.py's M step on an E step's results; cov_sums(weighted squares n x 2) adds a column in the implementation's order."""
    start = post[0] / post[0].sum()
    if x.size > 1:
        trans = stats[4:8].reshape(2, 2)
        rows = trans.sum(axis=1, keepdims=True)
        trans = np.where(rows > 0, trans / np.where(rows > 0, rows, 1.0), 0.5)
    else:
        trans = np.full((2, 2), 0.5)
    w = stats[0:2]
    means = stats[2:4] / w
    covars = np.maximum((covars_prior + cov_sums(post * (x[:, None] - means[None, :]) ** 2)) / w, 1e-300)
    return means, covars, start, trans


def host_cov_sums(sq):
    """hmm_host.h: every piece of n / 2048 added window by window, then the pieces in order."""
    n = sq.shape[0]
    P = min(256, max(1, n // 2048))
    out = []
    for j in (0, 1):
        col, total = sq[:, j].tolist(), 0.0
        for p in range(P):
            s = 0.0
            for v in col[n * p // P:n * (p + 1) // P]:
                s += v
            total += s
        out.append(total)
    return np.array(out)


@pytest.mark.parametrize("name", ["clean", "outlier", "n2"])
def test_the_hook_is_the_fit_host(name):
    x = H.fit_input(name)
    start = GaussianHMM2(native=True, n_iter=0).fit(x)
    post, stats, ll = start.e_step(x)
    one = GaussianHMM2(native=True, n_iter=1).fit(x)
    assert one.n_iter_ == 1 and one.loglik_ == ll
    for got, want in zip((one.means_, one.covars_, one.startprob_, one.transmat_), m_step(x, post, stats, host_cov_sums)):
        assert np.array_equal(np.asarray(got), np.asarray(want)), name
