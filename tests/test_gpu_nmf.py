"""NMF on the GPU (csrc/nmf_kernels.h through frisk_amd.projection.NMF / nmf): the two products against long double within the
summation-order-free bound gamma(len) |X| |Q|, single steps from every recorded sklearn state (tests/golden/nmf,
tools/make_golden_nmf.py) within the derived forward-error bound of tests/nmf_oracle.step_bound, full runs against sklearn's
(iteration counts equal; Y and components within 16 x the CPU-measured gap of two double implementations), determinism and
resumability, exact zeros, the argument checks of the C ABI, one product and one step at n = 20 000, and the CLI end to end.

Measured on an MI355X: worst |device - sklearn| / bound over every recorded state 0.063 (states), 0.015 (violation); full-run
gaps to sklearn at most 4.8e-14 (components) and 1.1e-14 (Y) against allowances of 1e-12 .. 4.6e-12 and 4.8e-13 .. 9.7e-13
(DESIGN.md section 9.4 has the table)."""
import ctypes as C
import json
import os
import pickle
import subprocess
import sys
import time

import numpy as np
import pytest

import nmf_oracle as NO
from golden_util import GOLD, INPUTS

pytestmark = pytest.mark.gpu

G = NO.golden()
CASES = sorted(G["cases"])
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LD = np.longdouble


def run_tol(g, what, ref):
    """16 x max(run_gap, 1e-13 max|ref|): run_gap is the CPU-measured distance of sklearn's run from the oracle's pairwise-order
    run; the device's summation order differs from both."""
    return 16 * max(g["run_gap"][what], 1e-13 * float(np.abs(ref).max()))


def _ratio(err, b):
    return float(np.max(err[b > 0] / b[b > 0], initial=0.0))


# ------------------------------------------------------------------------------------------------ products
def _check_products(X, ps, seed):
    from frisk_amd.projection import NMF
    n, f = X.shape
    rs = np.random.RandomState(seed)
    Xl, aX = X.astype(LD), np.abs(X)
    with NMF(X, 1) as h1, NMF(X, 1) as h2:
        for p in ps:
            Qf, Qn = rs.normal(size=(f, p)), rs.normal(size=(n, p))
            Y, Z = h1.xq(Qf), h1.xtq(Qn)
            assert Y.tobytes() == h2.xq(Qf).tobytes() and Z.tobytes() == h2.xtq(Qn).tobytes()
            assert Y.tobytes() == h1.xq(Qf).tobytes() and Z.tobytes() == h1.xtq(Qn).tobytes()
            eY = np.abs(Y.astype(LD) - Xl @ Qf.astype(LD)).astype(np.float64)
            eZ = np.abs(Z.astype(LD) - Xl.T @ Qn.astype(LD)).astype(np.float64)
            # the long-double reference itself is exact to ~len 2^-64 |X| |Q|: a 2^-11 share of the double bound
            assert np.all(eY <= NO.gamma(f) * (1 + 2.0 ** -10) * (aX @ np.abs(Qf))), (n, f, p)
            assert np.all(eZ <= NO.gamma(n) * (1 + 2.0 ** -10) * (aX.T @ np.abs(Qn))), (n, f, p)


@pytest.mark.parametrize("case", CASES)
def test_products_match_long_double_on_the_golden_inputs(case):
    _check_products(NO.arrays(G, case)["X"], [1, 2, 3, 8, 9, 16, 17, 26], 1)


@pytest.mark.parametrize("n,f", [(1, 1), (3, 65), (64, 64), (257, 129), (8193, 70), (9000, 3)])
def test_products_at_wave_block_and_split_edges(n, f):
    """rows per wave (4, 2, 1), 64-feature lanes, and XT Q' from one split to the cap of 256 with a short last split"""
    X = np.abs(np.random.RandomState(n + f).normal(size=(n, f)))
    _check_products(X, [1, 2, 5, 12, 16, 26], 2)


# ------------------------------------------------------------------------------------------------ single steps
@pytest.mark.parametrize("case", CASES)
def test_steps_match_sklearn_states(case):
    """for every recorded (W_t, H_t): set; step gives sklearn's (W_t+1, H_t+1) and violation within nmf_oracle.step_bound; the
    same for the recorded transform steps with H fixed, through transform_prepare"""
    from frisk_amd.projection import NMF
    g, a = G["cases"][case], NO.arrays(G, case)
    X = a["X"]
    worst = worst_v = 0.0
    with NMF(X, g["d"]) as h:
        for k in range(len(a["fit_t"])):
            h.set(a["fit_W"][k], a["fit_H"][k])
            v = h.step(True)
            W1, H1 = h.get()
            bW, bH, bv = NO.step_bound(X, a["fit_W"][k], a["fit_H"][k])
            worst = max(worst, _ratio(np.abs(W1 - a["fit_W1"][k]), bW), _ratio(np.abs(H1 - a["fit_H1"][k]), bH))
            worst_v = max(worst_v, abs(v - a["fit_v"][k]) / bv)
            assert np.all(np.abs(W1 - a["fit_W1"][k]) <= bW) and np.all(np.abs(H1 - a["fit_H1"][k]) <= bH), (case, int(a["fit_t"][k]))
            assert abs(v - a["fit_v"][k]) <= bv
        h.set(H=a["components"])
        for k in range(len(a["tr_t"])):
            h.set(W=a["tr_W"][k])
            if k % 2 == 0:
                h.transform_prepare()           # (odd k: the step before left the frozen products valid)
            v = h.step(False)
            W1, H1 = h.get()
            bW, _bH, bv = NO.step_bound(X, a["tr_W"][k], a["components"], update_H=False)
            worst = max(worst, _ratio(np.abs(W1 - a["tr_W1"][k]), bW))
            worst_v = max(worst_v, abs(v - a["tr_v"][k]) / bv)
            assert np.array_equal(H1, a["components"])
            assert np.all(np.abs(W1 - a["tr_W1"][k]) <= bW) and abs(v - a["tr_v"][k]) <= bv
    print("%s: worst step ratio %.3g, worst violation ratio %.3g" % (case, worst, worst_v))
    assert worst <= 1.0 and worst_v <= 1.0


def test_step_through_the_abi_arrays_equals_the_resident_state():
    from frisk_amd import _ffi
    from frisk_amd.projection import NMF
    g, a = G["cases"]["odd"], NO.arrays(G, "odd")
    p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    with NMF(a["X"], g["d"]) as h:
        h.set(a["W0"], a["H0"])
        v1 = h.step(True)
        W1, H1 = h.get()
        W, H, v = a["W0"].copy(), np.ascontiguousarray(a["H0"]).copy(), C.c_double()
        assert _ffi.lib().frisk_nmf_step(h._h, p(W), p(H), 1, C.byref(v)) == _ffi.OK
        assert W.tobytes() == W1.tobytes() and H.tobytes() == H1.tobytes() and v.value == v1
        # a frozen transform step equals one that recomputes H HT and X HT
        h.set(W=np.zeros_like(W1))
        h.transform_prepare()
        va, Wa = h.step(False), h.get()[0]
        h.set(W=np.zeros_like(W1), H=H1)
        vb, Wb = h.step(False), h.get()[0]
        assert va == vb and Wa.tobytes() == Wb.tobytes()
        assert all(t >= 0 for t in h.last_ms())


# ------------------------------------------------------------------------------------------------ full runs
@pytest.mark.parametrize("case", CASES)
def test_full_run_matches_sklearn(case):
    from frisk_amd.projection import nmf
    g, a = G["cases"][case], NO.arrays(G, case)
    r = nmf(a["X"], g["d"], seed=g["seed"])
    gap_c, gap_y = float(np.abs(r.components - a["components"]).max()), float(np.abs(r.Y - a["Y"]).max())
    tol_c, tol_y = run_tol(g, "components", a["components"]), run_tol(g, "Y", a["Y"])
    print("%s: n_iter %d / %d (sklearn %d / %d); |components - sklearn| %.3g (allowed %.3g), |Y - sklearn| %.3g (allowed %.3g); "
          "|W0 - sklearn| %.3g, |H0 - sklearn| %.3g" % (case, r.n_iter, r.transform_n_iter, g["n_iter"], g["transform_n_iter"], gap_c,
                                                       tol_c, gap_y, tol_y, np.abs(r.W0 - a["W0"]).max(), np.abs(r.H0 - a["H0"]).max()))
    assert (r.n_iter, r.transform_n_iter) == (g["n_iter"], g["transform_n_iter"])
    assert len(r.violation_ratios) == r.n_iter and r.violation_ratios[0] == 1.0
    assert gap_c <= tol_c and gap_y <= tol_y
    assert set(r.timings) == {"init_ms", "fit_ms", "transform_ms"}
    # Y >= 0, and exactly 0 where sklearn's is, wherever the entry before its max(., 0) is further from 0 than the allowance
    assert r.Y.min() >= 0 and r.components.min() >= 0
    Ht = np.ascontiguousarray(a["components"].T)
    pre = np.zeros_like(a["Y"])
    NO.sweep(a["tr_W"][-1], Ht.T @ Ht, a["X"] @ Ht, pre=pre)
    clear = np.abs(pre) > tol_y
    assert np.array_equal((r.Y == 0)[clear], (a["Y"] == 0)[clear])
    assert g["zeros_in_Y"] == int((a["Y"] == 0).sum())


def test_runs_are_deterministic_and_resumable():
    from frisk_amd.projection import NMF, nmf
    g, a = G["cases"]["n257"], NO.arrays(G, "n257")
    X = a["X"]
    with NMF(X, g["d"]) as h:
        h.set(a["W0"], a["H0"])
        v10 = [h.step(True) for _ in range(10)]
        W10, H10 = h.get()
        h.set(a["W0"], a["H0"])
        v4 = [h.step(True) for _ in range(4)]
        W4, H4 = h.get()
    with NMF(X, g["d"]) as h:               # resumed in another handle from the state read back
        h.set(W4, H4)
        v6 = [h.step(True) for _ in range(6)]
        W6, H6 = h.get()
    assert v4 + v6 == v10 and W6.tobytes() == W10.tobytes() and H6.tobytes() == H10.tobytes()
    g, a = G["cases"]["odd"], NO.arrays(G, "odd")
    r1, r2 = nmf(a["X"], g["d"], seed=g["seed"]), nmf(a["X"], g["d"], seed=g["seed"])
    assert r1.Y.tobytes() == r2.Y.tobytes() and r1.components.tobytes() == r2.components.tobytes()
    assert r1.violation_ratios == r2.violation_ratios and (r1.n_iter, r1.transform_n_iter) == (r2.n_iter, r2.transform_n_iter)


# ------------------------------------------------------------------------------------------------ argument checks
def test_abi_rejects_bad_input():
    from frisk_amd import _ffi
    L, E = _ffi.lib(), _ffi.E_ARG
    p = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    X = np.random.RandomState(0).rand(20, 4)
    h = C.c_void_p()
    assert L.frisk_nmf_create(0, None, 20, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_nmf_create(0, p(X), 20, 4, 2, None) == E
    assert L.frisk_nmf_create(0, p(X), 0, 4, 2, C.byref(h)) == E and not h
    assert L.frisk_nmf_create(0, p(X), 20, 0, 2, C.byref(h)) == E and not h
    assert L.frisk_nmf_create(0, p(X), 20, 4, 0, C.byref(h)) == E and not h
    assert L.frisk_nmf_create(0, p(X), 20, 4, 17, C.byref(h)) == E and not h
    for bad_value in (np.nan, np.inf, -1e-300):
        bad = X.copy()
        bad[3, 1] = bad_value
        assert L.frisk_nmf_create(0, p(bad), 20, 4, 2, C.byref(h)) == E and not h
    v = C.c_double()
    assert L.frisk_nmf_xq(None, p(X), 2, p(X)) == E and L.frisk_nmf_xtq(None, p(X), 2, p(X)) == E
    assert L.frisk_nmf_step(None, None, None, 1, C.byref(v)) == E
    assert L.frisk_nmf_get(None, None, None) == E and L.frisk_nmf_set(None, None, None) == E
    assert L.frisk_nmf_transform_prepare(None) == E and L.frisk_nmf_last_ms(None, 0) == -1.0
    L.frisk_nmf_destroy(None)
    assert L.frisk_nmf_create(0, p(X), 20, 4, 2, C.byref(h)) == _ffi.OK and h
    try:
        Qf, Qn, Y, Z = np.ones((4, 26)), np.ones((20, 26)), np.empty((20, 26)), np.empty((4, 26))
        for fn, Q, out in ((L.frisk_nmf_xq, Qf, Y), (L.frisk_nmf_xtq, Qn, Z)):
            assert fn(h, p(Q), 0, p(out)) == E and fn(h, p(Q), 27, p(out)) == E
            assert fn(h, None, 2, p(out)) == E and fn(h, p(Q), 2, None) == E
            inf = Q.copy()
            inf[1, 1] = np.inf
            assert fn(h, p(inf), 26, p(out)) == E
            assert fn(h, p(Q), 26, p(out)) == _ffi.OK
        assert np.allclose(Y, X.sum(axis=1)[:, None]) and np.allclose(Z, X.sum(axis=0)[:, None])
        W, H = np.ones((20, 2)), np.ones((2, 4))
        nanW = W.copy()
        nanW[0, 0] = np.nan
        assert L.frisk_nmf_set(h, p(nanW), None) == E and L.frisk_nmf_set(h, None, p(np.full((2, 4), np.inf))) == E
        assert L.frisk_nmf_step(h, p(nanW), p(H), 1, C.byref(v)) == E
        assert L.frisk_nmf_step(h, p(W), p(H), 1, None) == E
        assert L.frisk_nmf_last_ms(h, 3) == -1.0 and L.frisk_nmf_last_ms(h, -1) == -1.0
        assert L.frisk_nmf_step(h, p(W), p(H), 1, C.byref(v)) == _ffi.OK
        assert np.isfinite(W).all() and np.isfinite(H).all() and np.isfinite(v.value)
    finally:
        L.frisk_nmf_destroy(h)


# ------------------------------------------------------------------------------------------------ size
@pytest.mark.timeout(30)
def test_twenty_thousand_rows_one_product_and_one_step():
    """n = 20 000, f = 2 772, d = 2: one X Q, one XT Q' and one step finish, finite, within 30 s (upload included)."""
    from frisk_amd.projection import NMF
    n, f, d = 20000, 2772, 2
    t0 = time.perf_counter()
    rs = np.random.RandomState(31)
    X = rs.random_sample((n, f))
    with NMF(X, d) as h:
        Y = h.xq(rs.random_sample((f, d)))
        Z = h.xtq(rs.random_sample((n, d)))
        h.set(rs.random_sample((n, d)), rs.random_sample((d, f)))
        v = h.step(True)
        ms = h.last_ms()
        W, H = h.get()
    took = time.perf_counter() - t0
    print("n = 20000, f = 2772, d = 2: X HT %.3f ms, XT W %.3f ms, step %.3f ms on the device; the whole test %.1f s" % (ms + (took,)))
    assert all(np.isfinite(A).all() for A in (Y, Z, W, H)) and np.isfinite(v) and v > 0
    assert W.min() >= 0 and H.min() >= 0 and Y.min() > 0 and Z.min() > 0
    assert took < 30.0


# ------------------------------------------------------------------------------------------------ CLI
E2E = json.load(open(os.path.join(GOLD, "mds.json")))["e2e"]        # the small FASTA and thresholds of the projection goldens


def _cli(tmp, argv):
    cmd = [sys.executable, "-m", "frisk_amd", "-H", os.path.join(INPUTS, E2E["fasta"]), "-t", str(tmp)] + argv
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


def test_cli_nmf_dumps_the_projection_and_changes_no_other_output(tmp_path):
    from frisk_amd.projection import nmf
    base = ["-m", "1", "-k", "4", "-w", "200", "-i", "100", "-F", str(E2E["forceThresholdKLD"]), "--pcaMin", "1", "--pcaMax", "3",
            "--gffOutfile", "a.gff3"]
    with_nmf, without = tmp_path / "N", tmp_path / "P"
    p = _cli(with_nmf, base + ["--runProjection", "NMF", "--projectionDims", "2", "--dumpPCAdata", "--cluster", "DBSCAN"])
    _cli(without, base)
    assert "NMF of %d x 44 k-mer proportions" % E2E["n_anomalous"] in p.stderr
    assert "--cluster is not available in this build" in p.stderr
    new = {"anomNMF", "anomLabels", "anomCounts"}
    assert set(os.listdir(with_nmf)) == set(os.listdir(without)) | new      # no cluster GFF3 among them
    assert not [name for name in os.listdir(with_nmf) if "cluster_labeled" in name]
    for name in os.listdir(without):
        assert open(with_nmf / name, "rb").read() == open(without / name, "rb").read(), name
    counts = pickle.load(open(with_nmf / "anomCounts", "rb"))
    Y = pickle.load(open(with_nmf / "anomNMF", "rb"))
    assert counts.shape == (E2E["n_anomalous"], 44)
    want = nmf(counts, 2, seed=0)
    assert Y.tobytes() == want.Y.tobytes() and Y.min() >= 0
