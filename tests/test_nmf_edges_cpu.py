"""The NMF edge cases of tests/nmf_edge_cases.py without a GPU: every case regenerates to its recorded sha256, really contains what
it claims (its dead component, zero columns, zero row, exact zeros on both branches of W[s][t] == 0), and two double
implementations of the step (numpy's BLAS order and pairwise-order sums) pass the very check the device gets, Reference.check, with
a worst ratio in (0, 1] per shape.  The new sklearn goldens (tools/make_golden_nmf.py --edges) are reproduced by the oracle, and
projection.nmf refuses all-zero components as sklearn's transform does."""
import hashlib
import os

import numpy as np
import pytest

import nmf_edge_cases as EC
import nmf_oracle as NO

SHAPES = list(EC.SHAPES)


def test_shapes_cover_every_form():
    ds = {d for _, _, d in SHAPES}
    assert ds == {1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16}
    for edge in (255, 256, 257):
        assert any(n == edge for n, _, _ in SHAPES) and any(f == edge for _, f, _ in SHAPES)
    assert max((n + 255) // 256 for n, _, _ in SHAPES if n < 2000) == 5
    splits = lambda n: -(-n // -(-n // min(256, -(-n // 32))))      # noqa: E731  State::xtq_splits().count
    assert splits(8161) == 256 and splits(8160) == 255 and splits(8193) == 249 and (8161, 5, 3) in SHAPES
    assert len({EC.case_id(s, st, u) for s in SHAPES for st, u in EC.cases(s)}) == 8 * (len(SHAPES) - 1) + 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_cases_hold_their_claims_and_two_double_steps_pass_the_device_check(shape):
    X, W0, H0 = EC.base(shape)
    recorded = EC.recorded_hashes()
    worst = 0.0
    for state, update_H in EC.cases(shape):
        cid = EC.case_id(shape, state, update_H)
        W, H = EC.with_state(W0, H0, state)
        assert EC.digest(X, W, H) == recorded[cid], cid
        ref = EC.Reference(X, W, H, update_H)
        ref.claims(state)
        # the reference alone: its own left-out share is under the cap
        own = ref.check(ref.Wl.astype(np.float64), ref.Hl.astype(np.float64), float(ref.vl))
        line = []
        for how in ("blas", "pairwise"):
            W1, H1, v = NO.step(X, W, H, update_H, how=how)
            r = ref.check(W1, H1, float(v))
            assert r["ratio"] <= 1.0 and r["ratio_v"] <= 1.0
            worst = max(worst, r["ratio"], r["ratio_v"])
            line.append("%s %.3g / %.3g" % (how, r["ratio"], r["ratio_v"]))
        print("%s: state / violation ratio %s; left out %d of %d (cap %d), %d inside the zero rows and columns"
              % (cid, ", ".join(line), own["left_out"], own["outside"], int(EC.LEFT_OUT_CAP * own["outside"]), own["left_in"]))
    print("%dx%dx%d: worst ratio %.3g" % (shape + (worst,)))
    assert 0 < worst <= 1.0


# ------------------------------------------------------------------------------------------------ the second golden table
GE = NO.golden("nmf_edges")
ECASES = sorted(GE["cases"])


def run_tol(g, what, ref):
    """The full-run yardstick of tests/test_nmf_cpu.py: 16 x max(run_gap, 1e-13 max|ref|)."""
    return 16 * max(g["run_gap"][what], 1e-13 * float(np.abs(ref).max()))


def test_edge_goldens_are_what_they_claim():
    assert GE["sklearn"].startswith("1.7") and (GE["tol"], GE["max_iter"], GE["dir"]) == (1e-4, 200, "nmf_edges")
    # f = 1 with d = 1: the nndsvda start of a rank-1 X is already the solution, sklearn's violations are rounding noise (1e-14)
    # and decide its iteration count at every seed: nothing another implementation could be held to
    assert GE["left_out"] == ["f1"] and set(ECASES) == {"d8", "d9", "absent", "dups", "rank1", "n1d1", "n1d3"}
    c = GE["cases"]
    assert (c["d8"]["d"], c["d9"]["d"]) == (8, 9) and c["d9"]["n"] < c["d9"]["f"]
    assert (c["n1d1"]["n"], c["n1d1"]["d"], c["n1d1"]["init"]) == (1, 1, "nndsvda")
    assert (c["n1d3"]["n"], c["n1d3"]["d"], c["n1d3"]["init"]) == (1, 3, "random")
    assert c["dups"]["null_triplets"] == [3, 4] and c["rank1"]["null_triplets"] == [1, 2]
    for case in ECASES:
        g, a = c[case], NO.arrays(GE, case)
        assert os.path.getsize(os.path.join(NO.GOLD, "nmf_edges", g["file"])) < 256 * 1024
        X = NO.make_X(g["X"])
        assert X.shape == (g["n"], g["f"]) and np.array_equal(X, a["X"]) and X.min() >= 0
        assert hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest() == g["X"]["sha256"]
        for ratios in (a["ratios"], a["tr_ratios"]):
            assert all(abs(r - GE["tol"]) / GE["tol"] >= 1e-3 for r in ratios[-2:])
        assert len(a["ratios"]) == g["n_iter"] and len(a["tr_ratios"]) == g["transform_n_iter"]
        for ts, T in ((a["fit_t"], g["n_iter"]), (a["tr_t"], g["transform_n_iter"])):
            assert ts.tolist() == sorted({0, T // 2} | set(range(max(0, T - 3), T)))
        assert np.array_equal(a["fit_H1"][-1], a["components"]) and np.array_equal(a["tr_W1"][-1], a["Y"])
        assert not np.any(a["tr_W"][0]) and np.array_equal(a["fit_W"][0], a["W0"]) and np.array_equal(a["fit_H"][0], a["H0"])
        assert g["zeros_in_Y"] == int((a["Y"] == 0).sum())
        if g["init"] == "nndsvda":
            assert g["cut_margin"] > 1e-9 and g["split_margin"] > 1e-9
            # everything a null triplet puts into the split lies below the cut: those components start from the mean of X
            Wr, Hr, _ms = NO.nndsvd_raw(a["U"], a["S"], a["V"])
            for j in g["null_triplets"]:
                assert a["S"][j] < 1e-12 * a["S"][0] and max(Wr[:, j].max(), Hr[j].max()) < 1e-6 - 1e-9
                assert np.all(a["W0"][:, j] == X.mean()) and np.all(a["H0"][j] == X.mean())
    a = NO.arrays(GE, "absent")
    assert int((~a["X"].any(axis=0)).sum()) == 3 and int((~a["X"].any(axis=1)).sum()) == 1
    assert len(np.unique(NO.arrays(GE, "dups")["X"], axis=0)) == 3
    assert np.linalg.matrix_rank(NO.arrays(GE, "rank1")["X"]) == 1
    assert (NO.arrays(GE, "rank1")["Y"] == 0).all(axis=0).any()        # sklearn leaves a whole column of Y zero


@pytest.mark.parametrize("case", ECASES)
def test_oracle_reproduces_the_edge_goldens(case):
    """start (the null triplets of a rank-deficient X excepted: rounding noise), every recorded step within the two-sided
    bound, and the whole run, as tests/test_nmf_cpu.py does for the first table"""
    g, a = GE["cases"][case], NO.arrays(GE, case)
    X = a["X"]
    if g["init"] == "nndsvda":
        U, S, V = NO.randomized_svd(X, g["d"], g["seed"])
        live = [j for j in range(g["d"]) if j not in g["null_triplets"]]
        for got, want in ((U[:, live], a["U"][:, live]), (S, a["S"]), (V[live], a["V"][live])):
            assert np.abs(got - want).max() <= 1e-14
    W0, H0 = NO.initialize(X, g["d"], g["seed"])
    assert np.array_equal(W0 == X.mean(), a["W0"] == X.mean()) and np.array_equal(H0 == X.mean(), a["H0"] == X.mean())
    assert np.abs(W0 - a["W0"]).max() <= 1e-14 and np.abs(H0 - a["H0"]).max() <= 1e-14
    worst = 0.0
    for k in range(len(a["fit_t"])):
        W1, H1, v = NO.step(X, a["fit_W"][k], a["fit_H"][k])
        bW, bH, bv = NO.step_bound(X, a["fit_W"][k], a["fit_H"][k])
        for got, want, b in ((W1, a["fit_W1"][k], bW), (H1, a["fit_H1"][k], bH)):
            err = np.abs(got - want)
            assert np.all(err <= b)
            worst = max(worst, float(np.max(err[b > 0] / b[b > 0], initial=0.0)))
        assert abs(v - a["fit_v"][k]) <= bv
    for k in range(len(a["tr_t"])):
        W1, _H, v = NO.step(X, a["tr_W"][k], a["components"], update_H=False)
        bW, _bH, bv = NO.step_bound(X, a["tr_W"][k], a["components"], update_H=False)
        assert np.all(np.abs(W1 - a["tr_W1"][k]) <= bW) and abs(v - a["tr_v"][k]) <= bv
    r = NO.fit_transform(X, g["d"], g["seed"])
    assert (r["n_iter"], r["transform_n_iter"]) == (g["n_iter"], g["transform_n_iter"])
    assert np.abs(r["components"] - a["components"]).max() <= run_tol(g, "components", a["components"])
    assert np.abs(r["Y"] - a["Y"]).max() <= run_tol(g, "Y", a["Y"])
    assert np.abs(np.array(r["ratios"]) - a["ratios"]).max() <= 1e-9
    print("%s: worst oracle step ratio %.3g" % (case, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the package's driver
def _numpy_nmf(monkeypatch):
    """projection.nmf with tests/test_nmf_cpu.NumpyHandle in place of the device handle."""
    from frisk_amd import projection as P
    from test_nmf_cpu import NumpyHandle
    real = P.NMF

    class Handle(NumpyHandle):
        def __init__(self, X, d, device=0):
            self.X, (self.n, self.f), self.dims = X, X.shape, d
            self.W, self.H = np.zeros((self.n, d)), np.zeros((d, self.f))
            self.iterate = lambda *a, **k: real.iterate(self, *a, **k)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def transform_prepare(self):
            pass

    monkeypatch.setattr(P, "NMF", Handle)
    return P.nmf


@pytest.mark.parametrize("case", ECASES)
def test_package_driver_on_a_numpy_handle_runs_the_edge_goldens(case, monkeypatch):
    nmf = _numpy_nmf(monkeypatch)
    g, a = GE["cases"][case], NO.arrays(GE, case)
    r = nmf(a["X"], g["d"], seed=g["seed"])
    assert (r.n_iter, r.transform_n_iter) == (g["n_iter"], g["transform_n_iter"])
    assert np.abs(r.components - a["components"]).max() <= run_tol(g, "components", a["components"])
    assert np.abs(r.Y - a["Y"]).max() <= run_tol(g, "Y", a["Y"])


@pytest.mark.parametrize("shape,d", [((6, 4), 2), ((1, 1), 1), ((3, 5), 4)])
def test_all_zero_components_raise_as_sklearns_transform_does(shape, d, monkeypatch):
    """sklearn 1.7.2: NMF(d, init=None).fit(X).transform(X) on an all-zero X raises this from _check_init(H, ...)"""
    nmf = _numpy_nmf(monkeypatch)
    with pytest.raises(ValueError, match=r"^Array passed to NMF \(input H\) is full of zeros\.$"):
        nmf(np.zeros(shape), d)
    assert nmf(np.eye(3), 2).components.any()
