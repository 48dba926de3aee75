"""The NMF kernels (csrc/nmf_kernels.h) driven with chosen states where they change form.

1. Single steps from the states of tests/nmf_edge_cases.py (16 shapes: every nmf_sweep<DMAX> at both edges of its range of d, the
   W and the H sweep on and across the 256-row block edge and over up to 33 blocks, XT W inside a step at exactly 256 row splits
   and at the capped split count; dead, revived and skipped components; all-zero rows and columns of X) against the long-double
   step of tests/nmf_oracle.py.  The tolerance is nmf_oracle.step_bound(..., sides=1), ONE double implementation against exact
   arithmetic, times the (1 + 2^-10) of the long-double reference's own rounding; it holds no measured constant.  Where the bound
   is 0 the device must return the input's bits.  nmf_edge_cases.Reference.check is the assertion, the same one that two CPU
   double implementations pass in tests/test_nmf_edges_cpu.py.  A frozen step runs with and without transform_prepare, a full step
   also after a prepare, and a second handle must give the same bits.
2. History independence: a seeded walk of 41 operations on one handle; every step must equal, bit for bit, the same step from
   the same state on a fresh handle.  Every sum has a fixed order, so only a stale or missing product can differ.
3. Full runs and recorded single steps of the second golden table (tests/golden/nmf_edges.json, tools/make_golden_nmf.py --edges:
   d = 8 and 9, absent k-mers, duplicated rows, rank 1, n = 1) against sklearn, by the rules of tests/test_gpu_nmf.py.
4. projection.nmf on an all-zero X raises as sklearn's transform does; f = 1 runs to the factorisation; a frozen step does not
   read X again (timed against what reading X must cost).

Measured on an MI355X (worst |device - long double| / bound per shape, state / violation; left out by the zero-pattern rule
outside the all-zero rows and columns of X, of the entries there, over the shape's cases, against the cap of 0.1 %):
  shape (n x f x d)  state     violation  left out
  1 x 1 x 1          0.069     0.068      0 of 16
  2 x 3 x 7          0.022     0.0015     0 of 280
  255 x 70 x 8       0.013     1.0e-04    0 of 20 288
  256 x 64 x 9       0.014     9.6e-06    0 of 22 536
  257 x 65 x 16      0.012     4.9e-06    0 of 40 320
  513 x 63 x 15      0.016     1.1e-05    0 of 68 280
  70 x 255 x 8       0.0042    4.9e-05    0 of 19 072
  64 x 256 x 9       0.0026    2.7e-05    0 of 21 096
  65 x 257 x 4       0.0032    3.7e-04    0 of 9 440
  63 x 769 x 5       0.0011    4.1e-05    0 of 30 160
  300 x 300 x 2      0.0028    5.7e-04    0 of 9 104
  300 x 300 x 3      0.0029    2.8e-04    0 of 13 656
  1025 x 40 x 6      0.021     8.9e-05    0 of 50 880
  8161 x 5 x 3       0.127     2.8e-05    0 of 195 936
  8193 x 6 x 2       0.117     6.2e-05    0 of 131 152
  1100 x 2772 x 2    0.00031   1.8e-07    0 of 7 188
Second golden table, worst |device - sklearn| / two-sided bound over the recorded steps (state / violation) and the full run's
gaps to sklearn (components / Y, against their allowances):
  absent  0.020 / 0.0029   3.9e-14 of 4.2e-12 / 2.2e-15 of 3.1e-13
  d8      0.022 / 0.0003   8.4e-14 of 4.1e-12 / 1.5e-14 of 7.2e-13
  d9      0.010 / 0.0007   1.0e-14 of 1.2e-12 / 3.9e-15 of 6.9e-13
  dups    0.018 / 0.013    2.1e-14 of 3.2e-12 / 5.3e-15 of 3.2e-13
  n1d1    0.017 / 0.020    2.8e-17 of 5.9e-13 / 0 of 9.6e-13
  n1d3    0.017 / 0.011    6.7e-16 of 3.4e-12 / 1.4e-15 of 6.2e-13
  rank1   0.034 / 0.0021   1.1e-12 of 8.6e-12 / 1.7e-15 of 5.0e-13
"""
import ctypes as C

import numpy as np
import pytest

import nmf_edge_cases as EC
import nmf_oracle as NO

pytestmark = pytest.mark.gpu

SHAPES = list(EC.SHAPES)


# ------------------------------------------------------------------------------------------------ 1. chosen states
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_steps_from_chosen_states_match_the_long_double_step(shape):
    from frisk_amd.projection import NMF
    X, W0, H0 = EC.base(shape)
    worst = worst_v = 0.0
    left = outside = 0
    with NMF(X, shape[2]) as h1, NMF(X, shape[2]) as h2:
        for state, update_H in EC.cases(shape):
            cid = EC.case_id(shape, state, update_H)
            W, H = EC.with_state(W0, H0, state)
            ref = EC.Reference(X, W, H, update_H)
            runs = []
            for h, prepare in ((h1, False), (h1, True), (h2, False)):
                h.set(W, H)
                if prepare:
                    h.transform_prepare()
                v = h.step(update_H)
                runs.append(h.get() + (v,))
            W1, H1, v = runs[0]
            for Wb, Hb, vb in runs[1:]:
                assert Wb.tobytes() == W1.tobytes() and Hb.tobytes() == H1.tobytes() and vb == v, cid
            r = ref.check(W1, H1, v)
            print("%s: worst ratio %.3g (state), %.3g (violation); left out %d of %d (cap %d), %d inside the zero rows and columns"
                  % (cid, r["ratio"], r["ratio_v"], r["left_out"], r["outside"], int(EC.LEFT_OUT_CAP * r["outside"]), r["left_in"]))
            worst, worst_v = max(worst, r["ratio"]), max(worst_v, r["ratio_v"])
            left, outside = left + r["left_out"], outside + r["outside"]
    print("%dx%dx%d: worst ratio %.3g (state), %.3g (violation); left out %d of %d" % (shape + (worst, worst_v, left, outside)))
    assert worst <= 1.0 and worst_v <= 1.0


# ------------------------------------------------------------------------------------------------ 2. history independence
WALK_LEN = 24      # every operation once and 7 more, before the required sequences are spliced in
REQUIRED = [["step_F", "set_H", "step_F"], ["step_F", "set_W", "step_F"], ["prepare", "xq", "xtq", "step_F"],
            ["prepare", "step_T", "step_F"], ["abi_H_F", "step_F"], ["abi_H_T", "step_F"]]
OPS = ["set_W", "set_H", "set_WH", "step_T", "step_F", "prepare", "xq", "xtq", "get",
       "abi_W_T", "abi_W_F", "abi_H_T", "abi_H_F", "abi_WH_T", "abi_WH_F", "abi__T", "abi__F"]


def _walk(seed):
    """WALK_LEN seeded operations with the required sequences spliced in between them, in a seeded order: 41 operations."""
    rs = np.random.RandomState(seed)
    ops = [OPS[k] for k in rs.permutation(np.concatenate([np.arange(len(OPS)), rs.randint(len(OPS), size=WALK_LEN - len(OPS))]))]
    at = sorted(rs.randint(WALK_LEN + 1, size=len(REQUIRED)).tolist(), reverse=True)
    for pos, k in zip(at, rs.permutation(len(REQUIRED))):
        ops[pos:pos] = REQUIRED[k]
    return ops


def _contains(log, seq):
    return any(log[k:k + len(seq)] == seq for k in range(len(log) - len(seq) + 1))


@pytest.mark.parametrize("case", ["odd", "n257"])
def test_a_step_does_not_depend_on_the_handles_history(case):
    """(67, 36, 3) and (257, 36, 5), the X of two goldens.  The walk's model of State::frozen: set(H) clears it, set(W) keeps it,
    transform_prepare sets it, a step leaves it at !update_H; the fresh handle prepares if and only if the walked step ran frozen."""
    from frisk_amd import _ffi
    from frisk_amd.projection import NMF
    g = NO.golden()
    X, d = NO.arrays(g, case)["X"], g["cases"][case]["d"]
    n, f = X.shape
    assert (n, f, d) == {"odd": (67, 36, 3), "n257": (257, 36, 5)}[case]
    rs = np.random.RandomState(n)
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)      # noqa: E731

    def draw(shape):
        """W in [0, 1), H in [0, 0.3 / d) so that W H is of the size of X (rows summing to 2 over 36 features) and a step moves
        entries both ways; a quarter exactly 0"""
        A = rs.random_sample(shape) * (1.0 if shape[0] == n else 0.3 / d)
        A[rs.random_sample(shape) < 0.25] = 0.0
        return A

    def one_step(h, W_in, H_in, update_H, abi):
        """The step as the walk asks for it; (W', H', violation) read back from the handle."""
        if abi:
            Wb, Hb, v = (None if W_in is None else W_in.copy()), (None if H_in is None else H_in.copy()), C.c_double()
            assert _ffi.lib().frisk_nmf_step(h._h, p(Wb), p(Hb), 1 if update_H else 0, C.byref(v)) == _ffi.OK
            W1, H1 = h.get()
            assert (Wb is None or Wb.tobytes() == W1.tobytes()) and (Hb is None or Hb.tobytes() == H1.tobytes())
            return W1, H1, v.value
        v = h.step(update_H)
        return h.get() + (v,)

    ops = _walk(n)
    assert len(ops) == 41 and all(_contains(ops, seq) for seq in REQUIRED)
    for kind in ("set_W", "set_H", "set_WH", "xq", "xtq", "get", "abi_W", "abi_H", "abi_WH", "abi__"):
        assert any(op.startswith(kind) for op in ops), kind
    frozen, steps, frozen_steps = False, 0, 0
    with NMF(X, d) as h:
        h.set(draw((n, d)), draw((d, f)))
        for k, op in enumerate(ops):
            if op == "set_W":
                h.set(W=draw((n, d)))
            elif op == "set_H":
                h.set(H=draw((d, f)))
                frozen = False
            elif op == "set_WH":
                h.set(draw((n, d)), draw((d, f)))
                frozen = False
            elif op == "prepare":
                h.transform_prepare()
                frozen = True
            elif op == "xq":
                h.xq(rs.normal(size=(f, rs.randint(1, 27))))
            elif op == "xtq":
                h.xtq(rs.normal(size=(n, rs.randint(1, 27))))
            elif op == "get":
                h.get()
            else:
                abi = op.startswith("abi")
                update_H = op.endswith("_T")
                W_in = draw((n, d)) if abi and "W" in op.split("_")[1] else None
                H_in = draw((d, f)) if abi and "H" in op.split("_")[1] else None
                Ws, Hs = h.get()                                    # the state the step starts from
                Ws, Hs = (Ws if W_in is None else W_in), (Hs if H_in is None else H_in)
                if H_in is not None:
                    frozen = False
                got = one_step(h, W_in, H_in, update_H, abi)
                with NMF(X, d) as fresh:
                    fresh.set(Ws, Hs)
                    if frozen:
                        fresh.transform_prepare()
                    want = one_step(fresh, None, None, update_H, False)
                where = (case, k, ops[max(0, k - 3):k + 1])
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), where
                assert got[2] == want[2], where
                if not update_H:
                    assert got[1].tobytes() == Hs.tobytes(), where
                assert float((got[0] > 0).mean()) > 0.1, where               # (the draws do not get W clamped away)
                steps, frozen_steps = steps + 1, frozen_steps + int(frozen)
                frozen = not update_H
    print("%s: %d operations, %d steps compared, %d of them on frozen products" % (case, len(ops), steps, frozen_steps))
    assert steps >= 15 and frozen_steps >= 4


# ------------------------------------------------------------------------------------------------ 3. the second golden table
GE = NO.golden("nmf_edges")
ECASES = sorted(GE["cases"])


def run_tol(g, what, ref):
    """16 x max(run_gap, 1e-13 max|ref|), the yardstick of tests/test_gpu_nmf.py: run_gap is the CPU-measured distance of sklearn's
    run from the oracle's pairwise-order run."""
    return 16 * max(g["run_gap"][what], 1e-13 * float(np.abs(ref).max()))


def _ratio(err, b):
    return float(np.max(err[b > 0] / b[b > 0], initial=0.0))


@pytest.mark.parametrize("case", ECASES)
def test_edge_steps_match_sklearn_states(case):
    """tests/test_gpu_nmf.py::test_steps_match_sklearn_states on the second table: two double implementations, sides = 2"""
    from frisk_amd.projection import NMF
    g, a = GE["cases"][case], NO.arrays(GE, case)
    X = a["X"]
    worst = worst_v = 0.0
    with NMF(X, g["d"]) as h:
        for k in range(len(a["fit_t"])):
            h.set(a["fit_W"][k], a["fit_H"][k])
            v = h.step(True)
            W1, H1 = h.get()
            bW, bH, bv = NO.step_bound(X, a["fit_W"][k], a["fit_H"][k])
            eW, eH = np.abs(W1 - a["fit_W1"][k]), np.abs(H1 - a["fit_H1"][k])
            worst, worst_v = max(worst, _ratio(eW, bW), _ratio(eH, bH)), max(worst_v, abs(v - a["fit_v"][k]) / bv if bv else 0.0)
            assert np.all(eW <= bW) and np.all(eH <= bH) and abs(v - a["fit_v"][k]) <= bv, (case, int(a["fit_t"][k]))
        h.set(H=a["components"])
        for k in range(len(a["tr_t"])):
            h.set(W=a["tr_W"][k])
            if k % 2 == 0:
                h.transform_prepare()           # (odd k: the step before left the frozen products valid)
            v = h.step(False)
            W1, H1 = h.get()
            bW, _bH, bv = NO.step_bound(X, a["tr_W"][k], a["components"], update_H=False)
            eW = np.abs(W1 - a["tr_W1"][k])
            worst, worst_v = max(worst, _ratio(eW, bW)), max(worst_v, abs(v - a["tr_v"][k]) / bv if bv else 0.0)
            assert np.array_equal(H1, a["components"])
            assert np.all(eW <= bW) and abs(v - a["tr_v"][k]) <= bv, (case, int(a["tr_t"][k]))
    print("%s: worst step ratio %.3g, worst violation ratio %.3g" % (case, worst, worst_v))


@pytest.mark.parametrize("case", ECASES)
def test_edge_full_run_matches_sklearn(case):
    from frisk_amd.projection import nmf
    g, a = GE["cases"][case], NO.arrays(GE, case)
    r = nmf(a["X"], g["d"], seed=g["seed"])
    gap_c, gap_y = float(np.abs(r.components - a["components"]).max()), float(np.abs(r.Y - a["Y"]).max())
    tol_c, tol_y = run_tol(g, "components", a["components"]), run_tol(g, "Y", a["Y"])
    print("%s: n_iter %d / %d (sklearn %d / %d); |components - sklearn| %.3g (allowed %.3g), |Y - sklearn| %.3g (allowed %.3g); "
          "|W0 - sklearn| %.3g, |H0 - sklearn| %.3g" % (case, r.n_iter, r.transform_n_iter, g["n_iter"], g["transform_n_iter"], gap_c,
                                                       tol_c, gap_y, tol_y, np.abs(r.W0 - a["W0"]).max(), np.abs(r.H0 - a["H0"]).max()))
    assert (r.n_iter, r.transform_n_iter) == (g["n_iter"], g["transform_n_iter"])
    assert len(r.violation_ratios) == r.n_iter and r.violation_ratios[0] == 1.0
    assert gap_c <= tol_c and gap_y <= tol_y
    assert r.Y.min() >= 0 and r.components.min() >= 0
    Ht = np.ascontiguousarray(a["components"].T)
    pre = np.zeros_like(a["Y"])
    NO.sweep(a["tr_W"][-1], Ht.T @ Ht, a["X"] @ Ht, pre=pre)
    clear = np.abs(pre) > tol_y
    assert np.array_equal((r.Y == 0)[clear], (a["Y"] == 0)[clear])
    assert g["zeros_in_Y"] == int((a["Y"] == 0).sum())


# ------------------------------------------------------------------------------------------------ 4. the driver's edges
def test_all_zero_x_raises_as_sklearns_transform_does():
    from frisk_amd.projection import NMF, nmf
    for shape, d in (((6, 4), 2), ((1, 1), 1), ((3, 5), 4), ((300, 70), 9)):
        with pytest.raises(ValueError, match=r"^Array passed to NMF \(input H\) is full of zeros\.$"):
            nmf(np.zeros(shape), d)
    # and the step itself on an all-zero problem: every Hessian is 0, nothing moves, the violation is exactly 0
    with NMF(np.zeros((300, 70)), 9) as h:
        assert h.step(True) == 0.0 and h.step(False) == 0.0
        W, H = h.get()
        assert not W.any() and not H.any()


def test_one_feature_runs_to_the_factorisation():
    """f = 1, d = 1 has no sklearn golden (the start is already the solution and sklearn's iteration count is rounding noise,
    tests/test_nmf_edges_cpu.py); the run must still end, finite, at Y H = X to a few ulp."""
    from frisk_amd.projection import nmf
    X = 0.25 + np.random.RandomState(5).random_sample((40, 1))
    r = nmf(X, 1, seed=0)
    assert np.isfinite(r.Y).all() and r.Y.min() > 0 and r.components.shape == (1, 1) and r.components[0, 0] > 0
    assert np.abs(r.Y @ r.components - X).max() <= 8 * NO.EPS * X.max()


def test_a_frozen_step_does_not_read_x_again():
    """What State::frozen is for.  Results cannot show whether a step recomputed H HT and X HT (the same kernels give the same
    bits), last_ms()[0] can: it times the part of a step that holds those two products, and X HT reads X once.  At n = 20 000,
    f = 2 772, X is 443.5 MB, 175 MB more than the 256 MiB Infinity Cache can hold, and HBM3E delivers at most 8 TB/s, so a step
    that computes X HT takes at least 175.1e6 / 8e12 s = 21.9 us there, whatever the kernel.  A step that reuses the products
    records two events back to back.  Best of five each, so that one slow event pair decides nothing.  (Measured on an MI355X:
    96 us recomputing, 5.2 us frozen.)"""
    from frisk_amd.projection import NMF
    n, f, d = 20000, 2772, 2
    floor_ms = 1e3 * (n * f * 8 - 256 * 2 ** 20) / 8e12
    rs = np.random.RandomState(33)
    with NMF(rs.random_sample((n, f)), d) as h:
        h.set(rs.random_sample((n, d)), rs.random_sample((d, f)))
        fresh, frozen, prepared = [], [], []
        for _ in range(5):
            h.set(H=rs.random_sample((d, f)))
            h.step(False)                       # H is new: both products
            fresh.append(h.last_ms()[0])
            h.set(W=rs.random_sample((n, d)))   # keeps them
            h.step(False)
            frozen.append(h.last_ms()[0])
            h.set(H=rs.random_sample((d, f)))
            h.transform_prepare()
            h.step(True)                        # prepared: reused once more, then H moves
            prepared.append(h.last_ms()[0])
            h.step(False)
            fresh.append(h.last_ms()[0])
    print("X HT part of a step, ms, best of %d / %d / %d: recomputed %.4f, frozen %.4f, after transform_prepare %.4f; floor %.4f"
          % (len(fresh), len(frozen), len(prepared), min(fresh), min(frozen), min(prepared), floor_ms))
    assert min(fresh) >= floor_ms
    assert min(frozen) < floor_ms and min(prepared) < floor_ms
