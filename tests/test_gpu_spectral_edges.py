"""The spectral kernels (csrc/spectral_kernels.h) on generated inputs at every instantiation, tile and range edge, which the
seventeen goldens of tests/test_gpu_spectral.py do not reach: d above AFF_KC, gamma other than 1, every p of a product at several
row counts, row counts on every constant of the kernels, more than 32 and the capped number of row ranges of the degrees,
underflowing and subnormal affinities, and several isolated points.  tests/spectral_edge_cases.py has the inputs and the checks,
tests/test_spectral_edges_cpu.py the proof that the references alone stay inside every condition used here.

One helper, common(), applies to a handle on (Y, gamma):
  1 affinities  exact symmetry, zero diagonal, [0, 1]; |A0 - A_hp| <= HP.affinity_bound; [0, DBL_MIN] below the normal range;
  2 degrees     dd and n_isolated against the long-double column sums of the device's own A0 (valid in every regime), and, where
                the case promises no ambiguous column, the comparison of test_gpu_spectral.py::test_degrees against A_hp;
  3 matrix      M == SO.matrix(A0, dd) bit for bit, M == M.T, and the affinities on request leave the same M behind;
  4 products    per p: |Z - HP.product(M, Q)| <= (n + 2) eps64 (|M| |Q|); the same bytes twice; the same bytes as the NMF product
                X Q on X = M (projection.NMF(M, 1).xq), the summation order that spec_mq documents.
No bound holds a measured constant but C_EXP, which is reused as calibrated.  Every test prints the device's worst ratios to its
bounds (exp: in units of eps64 beside C_EXP = 4).

Measured on an MI355X: exp at most 0.249 of C_EXP = 4 in every case, as on the goldens (printed as 0 where the first term of the
affinity bound covers the whole error, as at d >= 15); |dd - sqrt(w)| at most 0.099 (n = 7) and the products at most 0.131
(n = 3, 7) of their bounds, both falling with n to 0.001 and 2e-5 at n = 8200; of the 25 552 exact affinities below DBL_MIN at
gamma = 1e3 the device returns 172 as subnormals and the rest as 0, of the 392 of the subnormal-sum case 100 and 292; the embeddings take 50, 33 and 26 iterations (1
where p = n) to sines 0.55 .. 0.64 of their bound.  The whole file takes 4.3 s, test_range_cap_above_8192 0.6 s.

Defects seeded one at a time into scratch copies of spectral_kernels.h, and what fails then:
  the chunk loop of the affinity stops after one chunk       test_dims_at_chunk_edges at d = 17 .. 64 (7 of its 10 cases)
  minus_gamma = -1.0                                          test_gamma (all 3), test_underflowing_affinities
  dispatch bounds p <= 9, p <= 17                             every test with p = 9 or 17 (37): all row counts, test_every_p, ...
  spec_degrees sums nsplit - 1 partials                       all 54
  spec_normalise writes r, not the mean                       47: all but n = 2, 3 (r == r' there) and the embeddings
  the staging write keeps stale values beyond `cols`          none, and none can: those columns meet entries of M that are
                                                              zero-filled too (c >= n), and the ABI refuses a non-finite Q, so
                                                              every such term is 0 x finite
  rows_per() from DEG_SPLITS alone (another valid order)      none: values are pinned within bounds, not a summation order
"""
import functools
import time

import numpy as np
import pytest

import spectral_edge_cases as EC
import spectral_oracle as SO
import spectral_oracle_hp as HP

pytestmark = pytest.mark.gpu

LD = EC.LD
C = EC.CASES


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(Y, A_hp, d2_hp) of a case: computed once, read-only."""
    Y = EC.inputs(C[cid])
    A_hp, d2 = HP.affinity(Y, C[cid].gamma)
    for a in (Y, A_hp, d2):
        a.setflags(write=False)
    return Y, A_hp, d2


def common(cid):
    """Checks 1 to 4 on a fresh handle of the case; returns (A0, dd, n_isolated, M, the products by p)."""
    from frisk_amd.projection import NMF, Spectral
    case = C[cid]
    Y, A_hp, d2 = reference(cid)
    products = {}
    with Spectral(Y, case.gamma) as h:
        M = h.matrix()
        A0 = h.affinity()
        dd, iso = h.degrees()
        assert h.matrix().tobytes() == M.tobytes()
        with NMF(M, 1) as x:
            def mq(Q):
                Z = h.mq(Q)
                assert Z.tobytes() == h.mq(Q).tobytes(), (cid, Q.shape[1])
                assert Z.tobytes() == x.xq(Q).tobytes(), (cid, Q.shape[1])
                products[Q.shape[1]] = (Q, Z)
                return Z
            r = EC.check_all(case, Y, A0, dd, iso, M, mq, ref=(A_hp, d2))
    assert sorted(products) == sorted(case.ps)
    print("%s: exp %.3f (C_EXP %.0f); |dd - sqrt(w)| %.3g, products %.3g of their bounds; %d isolated"
          % (cid, r["exp"], HP.C_EXP, r["degrees"], r["product"], iso))
    return A0, dd, iso, M, products


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", EC.ROW_NS)
def test_row_counts_at_edges(n):
    """d = 2, gamma = 1, p in {1, 5, 16, 17, 26} (p > n is legal for a product).  What each n is there for:
      2, 3, 7          fewer rows than one wave's R = 2 / R = 4 takes, than the 8 rows of an R = 2 block; p above n
      8 | 9            the 8 rows of a block of spec_mq<26, 2>: one block | a second one of one row
      15, 16 | 17      the 16 rows of a block of spec_mq<., 4> (two R = 2 blocks): full | one row into the next
      31, 32 | 33      DEG_MIN_ROWS: one range of the column sums | two ranges (17 + 16 rows)
      63, 64 | 65      the 64-tile of the affinity and the 64 lanes of a product: lanes without a column | a second tile
      127, 128 | 129   MQ_C, the 128 columns of an LDS stage: no zero-filled tail at 128 | a second stage of one column
      191, 192 | 193   three tiles; a second stage exactly half full at 192 (its second half-stage all zeros)
      255, 256 | 257   the 256-column blocks of colsum_part / spec_degrees / spec_normalise | a second block of one column
      511, 512 | 513   two column blocks, four stages, 16 ranges | 17 ranges
      1025             33 ranges (more than any golden's 21), 17 x 17 tiles, 9 stages, 5 column blocks"""
    common("rows-n%d" % n)


@pytest.mark.parametrize("d", EC.DIMS)
def test_dims_at_chunk_edges(d):
    """n = 70 (two tiles, the second ragged), p in {3, 26}; d on and around the multiples of AFF_KC = 16 up to the ABI's 64: the
    second to fourth trips of the chunk loop, the ragged last chunk (kc), its zero-filled columns (kin) and the barrier that lets
    P and Q be overwritten"""
    common("dims-d%d" % d)


@pytest.mark.parametrize("n", list(EC.EVERY_P))
def test_every_p(n):
    """every p from 1 to 26 at n = 333 (ragged against 8, 16, 64, 128 and 256): every q_step = 256 % p, col_step = 256 / p and
    carry of the staging, every dispatch bound; p in {4, 5, 8, 9, 16, 17, 26} at n = 50 (one partial stage, lanes 50..63 without
    a column) and n = 256 (no partial stage)"""
    products = common("p-n%d" % n)[4]
    assert sorted(products) == list(EC.EVERY_P[n])


# ------------------------------------------------------------------------------------------------ gamma and the range of exp
@functools.lru_cache(maxsize=None)
def gamma_one_affinities():
    from frisk_amd.projection import Spectral
    with Spectral(reference("gamma-1")[0], 1.0) as h:
        A = h.affinity()
    A.setflags(write=False)
    return A


@pytest.mark.parametrize("gamma", EC.GAMMAS)
def test_gamma(gamma):
    """n = 197 under gamma in {0.01, 0.5, 7.3}; and A0 is not that of gamma = 1 on the same Y, which a kernel that dropped gamma
    would return"""
    cid = "gamma-%g" % gamma
    A0 = common(cid)[0]
    assert np.array_equal(reference(cid)[0], reference("gamma-1")[0])
    assert np.any(A0 != gamma_one_affinities())


def test_gamma_one_handle_itself():
    """the handle test_gamma compares against gets the checks too"""
    assert common("gamma-1")[0].tobytes() == gamma_one_affinities().tobytes()


def _consistent_where_affinities_vanish(cid):
    """dd, n_isolated and M against the device's own A0 (checks 2 and 3 inside common), everything finite; returns the counts"""
    A0, dd, iso, M, products = common(cid)
    A_hp = reference(cid)[1]
    assert np.isfinite(M).all() and np.isfinite(dd).all() and np.all(dd > 0)
    for _Q, Z in products.values():
        assert np.isfinite(Z).all()
    off = ~np.eye(C[cid].n, dtype=bool)
    tiny = (A_hp < LD(HP.DBL_MIN)) & off
    print("%s: %d exact affinities below DBL_MIN, of which the device returned %d as 0 and %d as subnormals; %d isolated"
          % (cid, int(tiny.sum()), int((A0[tiny] == 0).sum()), int((A0[tiny] > 0).sum()), iso))
    return A0, dd, iso, M


def test_underflowing_affinities():
    """n = 197, gamma = 1e3: a third of the exact affinities are below DBL_MIN and no column is certainly isolated.  Checks 1 to 4
    in their regime-free form only; every entry of M and every product finite"""
    _consistent_where_affinities_vanish("underflow")


def test_a_column_with_a_subnormal_sum():
    """one point whose largest exact affinity is exp(-712) = 6.2e-310: the device may return subnormals or zeros for its column,
    and dd, n_isolated and M must follow whichever it returned"""
    j = EC.SUBNORMAL_ROW
    A0, dd, iso, M = _consistent_where_affinities_vanish("subnormal")
    assert iso == (0 if A0[j].any() else 1) and np.all(A0[j] <= HP.DBL_MIN)


@pytest.mark.parametrize("variant", list(EC.MOVED))
def test_several_isolated_points(variant):
    """n = 645; rows 3, 300 and 600 (three 256-column blocks of spec_degrees, so three blocks' atomicAdd) moved to 1e3 x (+-1, +-1):
    n_isolated == 3, dd == 1 at exactly those columns, their rows and columns of M zero, their rows of Z exactly 0.  Where two of
    the moved points coincide they are not isolated: their mutual affinity is 1, dd == 1 from w == 1, n_isolated == 1"""
    cid = "isolated-" + variant
    A0, dd, iso, M, products = common(cid)
    moved = [r for r, _ in C[cid].moved]
    isolated = list(EC.ISOLATED[variant])
    assert iso == len(isolated) == {"apart": 3, "coincide": 1}[variant]
    assert np.flatnonzero(dd == 1.0).tolist() == moved == [3, 300, 600]
    rest = np.setdiff1d(np.arange(C[cid].n), moved)
    assert not A0[np.ix_(moved, rest)].any() and not M[np.ix_(moved, rest)].any() and not M[np.ix_(rest, moved)].any()
    assert not M[isolated].any() and not M[:, isolated].any()
    for _Q, Z in products.values():
        assert np.all(Z[isolated] == 0.0)
    if variant == "coincide":
        assert A0[3, 300] == A0[300, 3] == 1.0 and M[3, 300] == M[300, 3] == 1.0
        assert np.count_nonzero(M[3]) == np.count_nonzero(M[300]) == 1
        for Q, Z in products.values():
            assert np.array_equal(Z[3], Q[300]) and np.array_equal(Z[300], Q[3])      # 1.0 x q plus zeros


# ------------------------------------------------------------------------------------------------ the embedding
@pytest.mark.parametrize("nk", list(EC.EMBEDDINGS), ids=lambda nk: "n%d-k%d" % nk)
def test_embedding_on_generated_blobs(nk):
    """spectral_embedding on the device's products against numpy.linalg.eigh of the host oracle's M: residuals <= SPECTRAL_TOL in
    fewer than SPECTRAL_MAX_ITER iterations, eigenvalues within res.max() + n eps64, and the subspace sine at most sqrt(k) res.max()
    / gap_k + n eps64 wherever gap_k >= 0.1 (not at 17 points with k = 16: gap 0.025, eigenvalues and residuals only).  (17, 3) has
    p = 13 of 17; (17, 16) and (3, 2) have p = n"""
    from frisk_amd import projection as P
    n, k = nk
    Y = EC.embedding_inputs(n, k)
    with P.Spectral(Y) as h:
        E, lam, res, it = P.spectral_embedding(h, k, EC.EMBED_SEED)
        dd, iso = h.degrees()
        assert h.timings["products"] == it
    A = SO.affinity(Y)
    dd_host = SO.degrees(A)[0]
    gap, ratio = EC.check_embedding(n, k, EC.EMBEDDINGS[nk], E, lam, res, it, dd, SO.matrix(A, dd_host), P.SPECTRAL_TOL,
                                    P.SPECTRAL_MAX_ITER)
    assert iso == 0 and (it == 1 or min(k + P.SPECTRAL_GUARD, n) < n)
    print("n %d, k %d: gap %.3g, %d iterations, residual %.3g, sine / bound %s" % (
        n, k, gap, it, res.max(), "not compared" if ratio is None else "%.3f" % ratio))


# ------------------------------------------------------------------------------------------------ the capped range count
def test_range_cap_above_8192():
    """n = 8200, d = 2: the DEG_SPLITS cap holds the range count at 256, the ranges grow to 33 rows and only 249 of them are
    launched and allocated (splits() < nsplit for the first time; below 8193 the cap cannot be reached).  Check 2 on every column,
    the column sums of the downloaded A0 accumulated in long double over chunks of 512 rows; checks 1, 3 and 4 (p = 26 and 16)
    and the symmetry of A0 and M on 64 sampled rows and the last 9, against the matching columns.  Measured on an MI355X: 0.6 s
    of wall time, 0.47 s of it the host's checks (the long-double column sums) and 0.07 s the two 538 MB downloads; the printed
    line has the split."""
    from frisk_amd.projection import Spectral
    t0 = time.perf_counter()
    case = C["cap"]
    n = case.n
    assert EC.splits(n) == 249 < EC.DEG_SPLITS and EC.rows_per(n) == 33 and n > 8192
    Y, rows = EC.inputs(case), EC.cap_rows()
    rs = np.random.RandomState(case.seed + 100)
    with Spectral(Y, case.gamma) as h:
        t1 = time.perf_counter()
        M = h.matrix()
        A0 = h.affinity()
        dd, iso = h.degrees()
        t2 = time.perf_counter()
        products = []
        for p in case.ps:
            Q = rs.normal(size=(n, p))
            Z = h.mq(Q)
            assert Z.tobytes() == h.mq(Q).tobytes()
            products.append((Q, Z))
        t3 = time.perf_counter()
    # 1 on the rows
    assert np.all(np.diagonal(A0) == 0.0) and A0.min() >= 0.0 and A0.max() <= 1.0
    assert np.array_equal(A0[rows], A0[:, rows].T) and np.array_equal(M[rows], M[:, rows].T)
    A_hp, d2 = EC.affinity_rows(Y, case.gamma, rows)
    r_exp = EC.check_affinity_values(A0[rows], A_hp, d2, case.d, case.gamma)
    # 2 on every column
    r_deg = EC.check_degrees_own(EC.column_sums_ld(A0, EC.CAP_CHUNK), dd, iso, n)
    assert iso == 0
    # 3 on the rows: scipy's entry and its mirror, from the row and from the column of A0
    s = (A0[rows] / dd) / dd[rows, None]
    st = (A0[:, rows].T / dd[rows, None]) / dd
    assert np.array_equal(M[rows], 0.5 * (s + st))
    # 4 on the rows
    r_mq = max(EC.check_product(M[rows], Q, Z[rows], n) for Q, Z in products)
    for _Q, Z in products:
        assert np.isfinite(Z).all()
    t4 = time.perf_counter()
    print("cap: exp %.3f (C_EXP %.0f); |dd - sqrt(w)| %.3g, products %.3g of their bounds; create %.2f s, downloads %.2f s, "
          "products %.2f s, checks %.2f s, in all %.2f s"
          % (r_exp, HP.C_EXP, r_deg, r_mq, t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0))
