"""Metric MDS on the GPU (csrc/mds_kernels.h through frisk_amd.projection.MDS and mds) against the extended-precision oracle of
tests/mds_oracle_hp.py at every launch edge: the cases of tests/mds_hp_cases.py, each compared as |got - oracle| / unit with the
allowed ratios of tests/golden/mds_hp.json (8 x what a float64 model reaches on the CPU, tests/test_mds_hp_cpu.py).  The
dissimilarities at the tile, chunk and width edges, plain, far from the origin, with copied rows and with rows 1e-9 apart; one
step at both ends of every mds_step instantiation's range and at every rows-per-block and 256-thread edge, from a uniform, a
settled, a far, a partly coincident and a wholly coincident configuration; the stress over 256 and 257 partials; the stop rule
decided on either side of the oracle's v_T, which pins the sum of squared distances; and the driver's first and last passes."""
import numpy as np
import pytest

import mds_hp_cases as K
import mds_oracle_hp as HP

pytestmark = pytest.mark.gpu

G = K.golden()
ALLOWED = G["allowed"]
DELTA = G["delta"]


# ------------------------------------------------------------------------------------------------ dissimilarities
@pytest.mark.parametrize("cid", [c.id for c in K.DIS])
def test_dissimilarities_against_oracle(cid):
    from frisk_amd.projection import MDS
    c = K.DIS_BY_ID[cid]
    X = c.X()
    assert K.sha(X) == G["dissimilarities"][cid]["X"]
    with MDS(X, 2) as h:
        D = h.dissimilarities()
    r = K.check_D(c, D, ALLOWED["D"])
    print("%s: worst D ratio %.3g (allowed %.3g)" % (cid, r, ALLOWED["D"]))


# ------------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("cid", [c.id for c in K.STEPS + K.REDUCTIONS])
def test_step_against_oracle(cid):
    """run(Y, 1, 0): X_1 against the oracle's step from Y on the device's own D, and the stress against the oracle's stress of
    that X_1 (the reduction cases: Y1 on rows 0, 255, 256, n - 2, n - 1, the stress over every block's partial)."""
    from frisk_amd.projection import MDS
    c = K.STEP_BY_ID[cid]
    X, Y = c.X(), c.Y()
    g = G["steps"][cid]
    assert [K.sha(X), K.sha(Y)] == [g["X"], g["Y"]]
    with MDS(X, c.d) as h:
        D = h.dissimilarities()
        Y1, s1, it, trace = h.run(Y, 1, 0.0)
    assert it == 1 and trace.tolist() == [s1]
    assert np.array_equal(D == 0.0, c.D0() == 0.0)
    r = K.check_step(c, D, Y, Y1, s1, ALLOWED)
    print("%s: worst ratio Y1 %.3g (allowed %.3g), stress %.3g (%.3g)" % (cid, r["Y1"], ALLOWED["Y1"], r["stress"], ALLOWED["stress"]))


# ------------------------------------------------------------------------------------------------ stop rule and driver
@pytest.mark.parametrize("cid", [c.id for c in K.STOPS])
def test_stop_rule_on_either_side_of_the_oracles_v(cid):
    """With eps = v_T (1 + delta) the run stops after pass T + 1 with X_{T+1}; with eps = v_T (1 - delta) it goes on.  v_T is
    the oracle's, from the device's own D; delta is 8 x the float64 model's worst relative error of v_T."""
    from frisk_amd.projection import MDS
    c = K.STOP_BY_ID[cid]
    X = c.X()
    assert [K.sha(X), K.sha(c.Y0())] == [G["stops"][cid][k] for k in ("X", "Y0")]
    with MDS(X, c.d) as h:
        D = h.dissimilarities()
        o = HP.run(c.Y0(), D, K.STOP_ITERS, 0.0)
        r = K.check_stop(c, o, DELTA, h.run, ALLOWED["Y1"])
        _Y, _s, _it, trace = h.run(c.Y0(), K.STOP_ITERS, 0.0)
    rv = max(K.v_error((trace[t - 1] - trace[t]) / float(o["sumsq"][t] / 2), o["v"][t]) for t in range(1, c.T + 1))
    print("%s: v_T = %.6g, margin %.3g, delta %.3g; Y ratio %.3g (allowed %.3g); (old - stress) / (oracle's sumsq / 2) within "
          "%.3g eps of v" % (cid, float(o["v"][c.T]), K.margin(o["v"], c.T), DELTA, r, ALLOWED["Y1"], rv))
    assert rv <= ALLOWED["v"]


@pytest.mark.parametrize("n,d", K.DRIVER_SHAPES)
def test_driver_edges(n, d):
    """max_iter = 1, max_iter = 2 with eps = 1e300, and the all-coincident start with eps = 0 through four passes."""
    from frisk_amd.projection import MDS, mds
    c = K.StepCase(n, d)
    with MDS(c.X(), d) as h:
        r = K.check_driver(n, d, h.dissimilarities(), h.run, ALLOWED)
    print("driver n%d_d%d: worst Y ratio %.3g (allowed %.3g)" % (n, d, r, ALLOWED["Y1"]))
    # the package's own entry: the starts it draws, one pass each
    res = mds(c.X(), d, seed=5, n_init=2, max_iter=1)
    rs = np.random.RandomState(5)
    starts = [rs.uniform(size=n * d).reshape(n, d) for _ in range(2)]
    with MDS(c.X(), d) as h:
        D = h.dissimilarities()
    assert res.n_iters == [1, 1] and res.best_start == int(np.argmin(res.stresses))
    o = HP.step(starts[res.best_start], D, sums=False)
    assert HP.ratio(res.Y, o["Y1"], o["u_Y1"]) <= ALLOWED["Y1"]


# ------------------------------------------------------------------------------------------------ determinism
def test_second_calls_are_bit_identical():
    """One case per kernel: the dissimilarities (pair_tile), the three mds_step instantiations, mds_sum_parts past 256 partials."""
    from frisk_amd.projection import MDS
    c = K.DIS_BY_ID["close/n129_f9"]
    with MDS(c.X(), 2) as h1, MDS(c.X(), 2) as h2:
        assert h1.dissimilarities().tobytes() == h2.dissimilarities().tobytes()
    for cid in ("settled/n257_d2", "pairs/n257_d5", "plain/n257_d17", "parts/n2049_d2"):
        c = K.STEP_BY_ID[cid]
        with MDS(c.X(), c.d) as h:
            a, b = h.run(c.Y(), 3, 0.0), h.run(c.Y(), 3, 0.0)
        with MDS(c.X(), c.d) as h:
            e = h.run(c.Y(), 3, 0.0)
        for x in (b, e):
            assert a[0].tobytes() == x[0].tobytes() and a[1] == x[1] and a[2] == x[2] == 3 and a[3].tobytes() == x[3].tobytes(), cid
