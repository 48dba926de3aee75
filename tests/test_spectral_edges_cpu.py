"""The spectral edge cases of tests/spectral_edge_cases.py without a GPU: the proof that the references alone stay inside every
condition tests/test_gpu_spectral_edges.py relies on, so that a failure there is the device's.
  * numpy's double exp over every case's exponents stays within C_EXP / 4 of the long-double exp: the calibration of C_EXP = 4
    (tests/spectral_oracle_hp.py, done on the goldens' gamma = 1, d <= 5) carries over to d up to 64 and gamma from 0.01 to 1e3;
  * each case holds what it promises: no ambiguous column, the isolated columns, the underflowing affinities;
  * the double oracle (tests/spectral_oracle.py, numpy's products) passes the very checks the device gets, check_all and
    check_embedding, and the table of embedding cases records the measured gaps;
  * the restated shape functions against values computed by hand.
Measured here: worst exp ratio 0.585 (rows-n1025; 0.562 over the d and gamma cases); gamma = 1e3 leaves 25 552 exact affinities
below DBL_MIN and a smallest exact column sum of 2.4e-48; gaps lambda_k - lambda_{k+1} of the embedding cases 0.61, 1.02, 1.16,
0.025 (17 points, k = 16: no subspace comparison) and 1.00."""
import numpy as np
import pytest

import spectral_edge_cases as EC
import spectral_oracle as SO
import spectral_oracle_hp as HP

LD = EC.LD
WHOLE = [c for c in EC.CASES if c != "cap"]


def test_shape_functions_against_hand_computed_values():
    """n: (rows per range, ranges).  2 and 32: one range; 33: two of 17 and 16; 65: ceil(65 / 32) = 3 ranges of 22, 22, 21;
    1025: 33 ranges of 32, the last of one row; 8192: the last n with 32-row ranges, 256 of them; 8193: the cap holds the count
    at 256, ceil(8193 / 256) = 33 rows, which only ceil(8193 / 33) = 249 ranges fill; 8448 = 256 x 33 fills all 256 again;
    50 000: ceil(50000 / 256) = 196 rows, ceil(50000 / 196) = 256 ranges."""
    want = {2: (2, 1), 32: (32, 1), 33: (17, 2), 65: (22, 3), 1025: (32, 33), 8192: (32, 256), 8193: (33, 249), 8448: (33, 256),
            50000: (196, 256)}
    for n, (rp, s) in want.items():
        assert (EC.rows_per(n), EC.splits(n)) == (rp, s), n
    for n in list(want) + list(EC.ROW_NS) + [EC.CAP_N, 645, 8191, 8194, 49999]:
        rp, s = EC.rows_per(n), EC.splits(n)
        assert 1 <= s <= EC.DEG_SPLITS and (s - 1) * rp < n <= s * rp          # every range holds a row, the ranges cover n
    assert EC.splits(EC.CAP_N) == 249 and EC.rows_per(EC.CAP_N) == 33
    assert max(EC.splits(n) for n in EC.ROW_NS) == 33


def test_case_table_is_the_one_asked_for():
    C = EC.CASES
    assert [C["rows-n%d" % n].ps for n in EC.ROW_NS] == [(1, 5, 16, 17, 26)] * 27
    assert {C[c].d for c in C if c.startswith("dims-")} == {1, 15, 16, 17, 31, 32, 33, 48, 63, 64}
    assert all(C[c].n == 70 and C[c].ps == (3, 26) for c in C if c.startswith("dims-"))
    assert C["p-n333"].ps == tuple(range(1, 27)) and C["p-n50"].ps == C["p-n256"].ps == (4, 5, 8, 9, 16, 17, 26)
    assert sorted(C[c].gamma for c in C if c.startswith("gamma-")) == [0.01, 0.5, 1.0, 7.3]
    assert (C["underflow"].n, C["underflow"].gamma, C["underflow"].clear) == (197, 1e3, False)
    assert len({C[c].seed for c in C if C[c].n == 197}) == 1                  # one Y under every gamma
    assert all(C[c].n == 645 for c in C if c.startswith("isolated-"))
    assert {r // 256 for r in EC.ISOLATED["apart"]} == {0, 1, 2}
    assert all(c.d == 2 and c.gamma == 1.0 for c in C.values() if c.id[:4] in ("rows", "p-n3", "p-n5", "p-n2", "isol", "cap"))
    assert list(EC.EMBEDDINGS) == [(333, 3), (50, 3), (17, 3), (17, 16), (3, 2)]
    rows = EC.cap_rows()
    assert len(rows) == len(set(rows.tolist())) == 73 and rows[-9:].tolist() == list(range(8191, 8200))


@pytest.mark.parametrize("cid", WHOLE)
def test_case_holds_its_promise_and_the_double_oracle_passes_the_device_checks(cid):
    case = EC.CASES[cid]
    n = case.n
    Y = EC.inputs(case)
    assert Y.shape == (n, case.d) and np.isfinite(Y).all()
    # exp: the calibration carries over
    ratio = HP.exp_ratio(-case.gamma * SO.sqdist(Y))
    worst_exp = float(ratio.max(initial=0.0))
    assert worst_exp <= HP.C_EXP / 4
    # the promises
    A_hp, d2 = HP.affinity(Y, case.gamma)
    w_hp = HP.degrees(A_hp)
    certain_zero = np.all(A_hp < EC.CERTAIN_ZERO, axis=0)
    off = ~np.eye(n, dtype=bool)
    if case.clear:
        assert np.all(certain_zero | (w_hp > LD(HP.DBL_MIN) * n))
    if cid.startswith("isolated-"):
        assert np.flatnonzero(certain_zero).tolist() == list(EC.ISOLATED[cid[9:]])
        moved = [r for r, _ in case.moved]
        rest = np.setdiff1d(np.arange(n), moved)
        assert np.all(A_hp[np.ix_(moved, rest)] < EC.CERTAIN_ZERO)              # the moved points see none of the others
        if cid == "isolated-coincide":
            assert A_hp[3, 300] == 1 and w_hp[3] == 1 and w_hp[300] == 1
    elif cid == "underflow":
        assert not certain_zero.any() and int((A_hp[off] < LD(HP.DBL_MIN)).sum()) > 1000
    elif cid == "subnormal":
        j = EC.SUBNORMAL_ROW
        assert not certain_zero.any() and 0 < w_hp[j] < LD(HP.DBL_MIN) and abs(float(np.sort(d2[j])[1]) - EC.SUBNORMAL_D2) < 1e-9
        assert np.all(np.delete(w_hp, j) > LD(HP.DBL_MIN) * n)
    else:
        assert not certain_zero.any()
        if case.gamma <= 1.0:
            assert float(A_hp[off].min()) >= HP.DBL_MIN                            # every affinity a normal double
    # the double oracle under the device's checks
    A = SO.affinity(Y, case.gamma)
    dd, iso = SO.degrees(A)
    M = SO.matrix(A, dd)
    r = EC.check_all(case, Y, A, dd, iso, M, lambda Q: M @ Q, ref=(A_hp, d2))
    print("%s: worst exp ratio %.3f; smallest exact off-diagonal affinity %.3g (%d below DBL_MIN), column sum %.3g; oracle exp "
          "%.3f, degrees %.3g, product %.3g of their bounds" % (cid, worst_exp, float(A_hp[off].min()), int((
              A_hp[off] < LD(HP.DBL_MIN)).sum()), float(w_hp.min()), r["exp"], r["degrees"], r["product"]))


def test_gamma_cases_differ_from_gamma_one():
    """what test_gamma's extra assertion needs: the affinities under each gamma are not those under gamma = 1"""
    Y = EC.inputs(EC.CASES["gamma-1"])
    A1 = SO.affinity(Y, 1.0)
    for g in EC.GAMMAS + (EC.UNDERFLOW_GAMMA,):
        assert np.array_equal(EC.inputs(EC.CASES["gamma-%g" % g if g != 1e3 else "underflow"]), Y)
        assert np.any(SO.affinity(Y, g) != A1)


def test_cap_case_on_its_rows():
    """n = 8200 is checked on 73 rows: exp over those rows' exponents, and the double oracle's rows under the row checks"""
    case = EC.CASES["cap"]
    Y, rows = EC.inputs(case), EC.cap_rows()
    d2 = EC.sqdist_rows(Y, rows, np.float64)
    worst = float(HP.exp_ratio(-case.gamma * d2).max())
    assert worst <= HP.C_EXP / 4
    A_hp, d2_hp = EC.affinity_rows(Y, case.gamma, rows)
    A = np.exp(-case.gamma * d2)
    A[np.arange(len(rows)), rows] = 0.0
    r = EC.check_affinity_values(A, A_hp, d2_hp, case.d, case.gamma)
    assert float(A_hp.sum(axis=1).min()) > case.n * HP.DBL_MIN
    print("cap: worst exp ratio %.3f on %d rows; oracle exp %.3f of C_EXP" % (worst, len(rows), r))


def test_row_references_are_the_whole_references_rows():
    case = EC.CASES["rows-n129"]
    Y, rows = EC.inputs(case), np.array([0, 5, 64, 128])
    A_hp, d2 = HP.affinity(Y, 0.5)
    Ar, d2r = EC.affinity_rows(Y, 0.5, rows)
    assert np.array_equal(Ar, A_hp[rows]) and np.array_equal(d2r, d2[rows])
    assert np.array_equal(EC.sqdist_rows(Y, rows, np.float64), SO.sqdist(Y)[rows])
    A = SO.affinity(Y)
    # chunked and whole long-double sums differ by their order only: n roundings of 2^-64 each way
    whole = EC.column_sums_ld(A)
    assert np.all(np.abs(EC.column_sums_ld(A, 50) - whole) <= 2 * 129 * LD(2.0) ** -64 * whole)


@pytest.mark.parametrize("nk", list(EC.EMBEDDINGS), ids=lambda nk: "n%d-k%d" % nk)
def test_embedding_cases_and_the_oracles_embedding(nk):
    """the gap of each case decides whether its subspace is compared, and SO.embedding meets the bounds the device is held to"""
    n, k = nk
    Y = EC.embedding_inputs(n, k)
    assert float(HP.exp_ratio(-SO.sqdist(Y)).max()) <= HP.C_EXP / 4
    A = SO.affinity(Y)
    dd, iso = SO.degrees(A)
    M = SO.matrix(A, dd)
    assert iso == 0
    E, lam, res, it = SO.embedding(M, dd, k, EC.EMBED_SEED)
    gap, ratio = EC.check_embedding(n, k, EC.EMBEDDINGS[nk], E, lam, res, it, dd, M)
    assert it == 1 or min(k + SO.GUARD, n) < n
    print("n %d, k %d: gap %.3g, %d iterations, residual %.3g, sine / bound %s" % (
        n, k, gap, it, res.max(), "not compared" if ratio is None else "%.3f" % ratio))
