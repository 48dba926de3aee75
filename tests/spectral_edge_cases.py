"""Generated inputs for the spectral kernels (csrc/spectral_kernels.h) at the shapes where they change form, and the checks one
handle's results get, whatever produced them.  Pure numpy, no device: tests/test_spectral_edges_cpu.py proves that the inputs meet
the conditions the checks rely on and runs the checks on the double oracle (tests/spectral_oracle.py), tests/
test_gpu_spectral_edges.py runs them on the device.  The references are the existing ones: tests/spectral_oracle_hp.py in long
double, tests/spectral_oracle.py in double.

Inputs (legacy RandomState streams and elementwise arithmetic only, so every machine draws the same bits): blobs() puts point i at
centre i % k, the centres normal x sep / sqrt(d), the points centre + spread / sqrt(d) x normal.  With spread = 0.3, sep = 1 the
squared distances are of order 1 to 10 for every d up to 64, so at gamma = 1 every affinity is a comfortably normal double; the
embedding cases use spread = 0.15, sep = 3, which separates the blobs (lambda_k - lambda_{k+1} near 1).

The checks (numbered as in the docstrings of the tests):
  1 affinities  A0 exactly symmetric, diagonal exactly 0, entries in [0, 1]; |A0 - A_hp| <= HP.affinity_bound (the roundings
                carried through the exponent plus C_EXP eps64 for exp); anything in [0, DBL_MIN] where the exact value is below the
                smallest normal double.
  2 degrees     against the long-double column sums w of the SAME A0 that was handed in, which is valid in every regime, subnormal
                and flushed entries included: w == 0 -> dd == 1.0 exactly and the column is counted in n_isolated; elsewhere
                |dd - sqrt(w)| <= ((n + 1) eps64 / 2 + ((n + 1) eps64)^2 + eps64) sqrt(w).  Any order of n non-negative double
                additions is within (n - 1) eps64 / 2 (1 + ...) of the exact sum (no addition of doubles underflows), so within
                (n + 1) eps64 with the long-double reference's own n 2^-64 to spare; sqrt halves a relative error (the square term
                covers the curvature) and adds one rounding.  Where the case promises that no column sits between "certainly
                isolated" and "comfortably normal", also the comparison of tests/test_gpu_spectral.py::test_degrees against A_hp.
  3 matrix      M == SO.matrix(A0, dd) bit for bit, and M == M.T.
  4 products    |Z - HP.product(M, Q)| <= (n + 2) eps64 (|M| |Q|) per entry.
"""
from collections import OrderedDict, namedtuple

import numpy as np

import spectral_oracle as SO
import spectral_oracle_hp as HP

LD = np.longdouble
EPS = HP.EPS
DBL_MIN = HP.DBL_MIN
CERTAIN_ZERO = LD(2.0) ** -1075         # below half the smallest subnormal: a double exp of it is 0 whatever the rounding
MIN_GAP = 0.1                           # the goldens' min_gap: below it the subspace of the top k is not compared

# ---------------------------------------------------------------------------------------------------------- shape functions
DEG_SPLITS, DEG_MIN_ROWS = 256, 32      # spectral_kernels.h


def rows_per(n):
    """State::splits().rows_per (RowSplits of analysis_common.h): rows per range of the column sums."""
    nsplit = min(DEG_SPLITS, -(-n // DEG_MIN_ROWS))
    return -(-n // nsplit)


def splits(n):
    """State::splits().count: the ranges that rows_per leaves, which is what `part` is sized by and the grid's y."""
    return -(-n // rows_per(n))


# ---------------------------------------------------------------------------------------------------------- inputs
def blobs(n, d, k, seed, spread=0.3, sep=1.0):
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(k, d)) * sep / np.sqrt(d)
    return centres[np.arange(n) % k] + spread / np.sqrt(d) * rs.normal(size=(n, d))


# id, n, d, gamma, the p of its products, whether it promises that no column is ambiguous, the seed of Y, rows moved far away
Case = namedtuple("Case", "id n d gamma ps clear seed moved")

ROW_NS = (2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1025)
ROW_PS = (1, 5, 16, 17, 26)
DIM_N, DIM_PS = 70, (3, 26)
DIMS = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64)
P_EDGES = (4, 5, 8, 9, 16, 17, 26)
EVERY_P = OrderedDict([(333, tuple(range(1, 27))), (50, P_EDGES), (256, P_EDGES)])
GAMMA_N, GAMMA_SEED, GAMMA_PS = 197, 4197, (3, 17)
GAMMAS = (0.01, 0.5, 7.3)
UNDERFLOW_GAMMA = 1e3
# One column between the regimes, which no case of the issue's list reaches (there the smallest exact column sum is still a normal
# double): row 100 is put at squared distance 712 from its nearest point, the one of largest x, and further from every other, so
# that its largest exact affinity is exp(-712) = 6.2e-310 and its exact column sum a subnormal double.  A device exp may return
# subnormals there or flush them: either way dd, n_isolated and M must agree with the A0 it returned.
SUBNORMAL_ROW, SUBNORMAL_D2 = 100, 712.0
ISOLATED_N, ISOLATED_PS = 645, (5, 26)
FAR = 1e3
MOVED = OrderedDict([
    ("apart", ((3, (FAR, FAR)), (300, (-FAR, FAR)), (600, (FAR, -FAR)))),           # three 256-column blocks of spec_degrees
    ("coincide", ((3, (FAR, FAR)), (300, (FAR, FAR)), (600, (FAR, -FAR)))),         # 3 and 300 see each other: affinity 1
])
ISOLATED = {"apart": (3, 300, 600), "coincide": (600,)}
CAP_N, CAP_PS, CAP_SAMPLE, CAP_TAIL, CAP_CHUNK = 8200, (26, 16), 64, 9, 512


def _cases():
    out = OrderedDict()

    def add(c):
        assert c.id not in out
        out[c.id] = c
    for n in ROW_NS:
        add(Case("rows-n%d" % n, n, 2, 1.0, ROW_PS, True, 1000 + n, ()))
    for d in DIMS:
        add(Case("dims-d%d" % d, DIM_N, d, 1.0, DIM_PS, True, 2000 + d, ()))
    for n, ps in EVERY_P.items():
        add(Case("p-n%d" % n, n, 2, 1.0, ps, True, 3000 + n, ()))
    add(Case("gamma-1", GAMMA_N, 2, 1.0, GAMMA_PS, True, GAMMA_SEED, ()))           # the handle the others must differ from
    for g in GAMMAS:
        add(Case("gamma-%g" % g, GAMMA_N, 2, g, GAMMA_PS, True, GAMMA_SEED, ()))
    add(Case("underflow", GAMMA_N, 2, UNDERFLOW_GAMMA, GAMMA_PS, False, GAMMA_SEED, ()))
    add(Case("subnormal", GAMMA_N, 2, 1.0, GAMMA_PS, False, GAMMA_SEED, ((SUBNORMAL_ROW, None),)))
    for name, moved in MOVED.items():
        add(Case("isolated-" + name, ISOLATED_N, 2, 1.0, ISOLATED_PS, True, 5645, moved))
    add(Case("cap", CAP_N, 2, 1.0, CAP_PS, False, 8200, ()))        # checked on row samples; no promise is needed or made
    return out


CASES = _cases()


def inputs(case):
    """Y (n x d) of a case."""
    Y = blobs(case.n, case.d, 3, case.seed)
    for row, at in case.moved:
        if at is None:
            j = int(np.argmax(np.delete(Y[:, 0], row)))
            j += j >= row
            at = (Y[j, 0] + np.sqrt(SUBNORMAL_D2), Y[j, 1])
        Y[row] = at
    return Y


def cap_rows():
    """The rows the n = 8200 case is checked on: 64 sampled ones and the last 9 (the ragged last wave and block of a product, the
    last tile of the affinity, the last range of the degrees)."""
    rs = np.random.RandomState(CAP_N)
    head = np.sort(rs.choice(CAP_N - CAP_TAIL, CAP_SAMPLE, replace=False))
    return np.concatenate([head, np.arange(CAP_N - CAP_TAIL, CAP_N)])


# (n, k) -> whether lambda_k - lambda_{k+1} >= MIN_GAP, so that the subspace is compared (tests/test_spectral_edges_cpu.py measures
# the gaps and holds this table to them).  p = min(k + 10, n): 13 of 333, of 50 and of 17, then p = n = 17 and p = n = 3.
EMBEDDINGS = OrderedDict([((333, 3), True), ((50, 3), True), ((17, 3), True), ((17, 16), False), ((3, 2), True)])
EMBED_SEED = 0


def embedding_inputs(n, k):
    return blobs(n, 2, k, 6000 + 100 * k + n, spread=0.15, sep=3.0)


# ---------------------------------------------------------------------------------------------------------- references
def sqdist_rows(Y, rows, dtype=LD):
    """The rows `rows` of HP.sqdist(Y) (or of SO.sqdist for dtype float64): the same sums in the same order."""
    Y = np.asarray(Y, dtype=np.float64).astype(dtype)
    s = np.zeros((len(rows), Y.shape[0]), dtype=dtype)
    for c in range(Y.shape[1]):
        t = Y[rows, None, c] - Y[None, :, c]
        s += t * t
    return s


def affinity_rows(Y, gamma, rows):
    """(A_hp, d2_hp) of HP.affinity restricted to `rows`."""
    d2 = sqdist_rows(Y, rows)
    A = np.exp(-LD(gamma) * d2)
    A[np.arange(len(rows)), rows] = LD(0)
    return A, d2


def column_sums_ld(A, chunk=None):
    """Long-double column sums of a double matrix; over row chunks where `chunk` is given, so that no n x n long-double array is
    formed."""
    if chunk is None:
        return A.astype(LD).sum(axis=0)
    w = np.zeros(A.shape[1], dtype=LD)
    for i0 in range(0, A.shape[0], chunk):
        w += A[i0:i0 + chunk].astype(LD).sum(axis=0)
    return w


# ---------------------------------------------------------------------------------------------------------- the checks
def check_affinity_values(A0, A_hp, d2_hp, d, gamma):
    """Check 1 but for the symmetry, on whole matrices or on matching rows of them; returns the worst ratio of exp's share."""
    assert np.all(A0 >= 0.0) and np.all(A0 <= 1.0)
    bound = HP.affinity_bound(A_hp, d2_hp, d, gamma)
    err = np.abs(A0.astype(LD) - A_hp).astype(np.float64)
    normal = A_hp >= LD(DBL_MIN)
    excess = err[normal] / (EPS * A_hp[normal].astype(np.float64)) - (d + 2) * gamma * d2_hp[normal].astype(np.float64)
    assert np.all(err <= bound), float((err / bound)[bound > 0].max())
    assert np.all(A0[~normal] <= DBL_MIN)
    return float(excess.max(initial=0.0))


def check_affinity(A0, A_hp, d2_hp, d, gamma):
    """Check 1."""
    assert np.array_equal(A0, A0.T) and np.all(np.diagonal(A0) == 0.0)
    return check_affinity_values(A0, A_hp, d2_hp, d, gamma)


def check_degrees_own(w, dd, iso, n):
    """Check 2 in its regime-free form; w: the long-double column sums of the A0 that dd was computed from.  Returns the worst
    |dd - sqrt(w)| / allowance."""
    zero = w == 0
    assert np.all(dd[zero] == 1.0) and iso == int(zero.sum()), (iso, int(zero.sum()))
    want = np.sqrt(w[~zero])
    rel = LD((n + 1) * EPS)
    allow = (rel / 2 + rel * rel + LD(EPS)) * want
    err = np.abs(dd[~zero].astype(LD) - want)
    assert np.all(err <= allow), float((err / allow).max())
    return float((err / allow).max(initial=0.0))


def check_degrees_hp(dd, iso, A_hp, bound, n):
    """tests/test_gpu_spectral.py::test_degrees, for a case that promises no ambiguous column."""
    certain_zero = np.all(A_hp < CERTAIN_ZERO, axis=0)
    assert iso == int(certain_zero.sum()) and np.all(dd[certain_zero] == 1.0)
    w_hp = HP.degrees(A_hp)[~certain_zero]
    assert np.all(w_hp > LD(DBL_MIN) * n)
    rel = ((n + 1) * EPS * w_hp + bound[:, ~certain_zero].sum(axis=0).astype(LD)) / w_hp
    want = np.sqrt(w_hp)
    err = np.abs(dd[~certain_zero].astype(LD) - want)
    assert np.all(err <= (rel / 2 + rel * rel + EPS) * want)


def check_matrix(A0, dd, M):
    """Check 3."""
    assert np.array_equal(M, M.T)
    assert np.array_equal(M, SO.matrix(A0, dd))
    assert np.isfinite(M).all()


def check_product(M_rows, Q, Z_rows, n):
    """Check 4 on whole matrices or on matching rows of M and Z; returns the worst ratio to the bound."""
    assert np.isfinite(Z_rows).all()
    err = np.abs(Z_rows.astype(LD) - HP.product(M_rows, Q)).astype(np.float64)
    bound = (n + 2) * EPS * (np.abs(M_rows) @ np.abs(Q))
    assert np.all(err <= bound), float((err[bound > 0] / bound[bound > 0]).max(initial=np.inf))
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def check_all(case, Y, A0, dd, iso, M, mq, ref=None):
    """Checks 1 to 4 of one case on (A0, dd, n_isolated, M) and the product function mq.  ref: (A_hp, d2_hp) where the caller has
    them already.  Returns the ratios to print."""
    n = case.n
    assert A0.shape == M.shape == (n, n) and dd.shape == (n,)
    A_hp, d2 = ref if ref is not None else HP.affinity(Y, case.gamma)
    out = OrderedDict()
    out["exp"] = check_affinity(A0, A_hp, d2, case.d, case.gamma)
    out["degrees"] = check_degrees_own(column_sums_ld(A0), dd, iso, n)
    if case.clear:
        check_degrees_hp(dd, iso, A_hp, HP.affinity_bound(A_hp, d2, case.d, case.gamma), n)
    check_matrix(A0, dd, M)
    rs = np.random.RandomState(case.seed + 100)
    worst = 0.0
    for p in case.ps:
        Q = rs.normal(size=(n, p))
        worst = max(worst, check_product(M, Q, mq(Q), n))
    out["product"] = worst
    return out


def top_eigenpairs(M):
    """(eigenvalues descending, eigenvectors to match) of numpy.linalg.eigh."""
    w, U = np.linalg.eigh(M)
    return w[::-1], U[:, ::-1]


def check_embedding(n, k, subspace, E, lam, res, it, dd, M_host, tol=SO.TOL, max_iter=SO.MAX_ITER):
    """An embedding (E, eigenvalues, residuals, iterations; dd what E's vectors were divided by) against eigh of the host oracle's
    M: residuals <= tol in fewer than max_iter iterations; eigenvalues within res.max() + n eps64; where the case compares the
    subspace (gap_k >= MIN_GAP), its sine at most sqrt(k) res.max() / gap_k + n eps64 - Davis-Kahan with the Frobenius norm of the
    k residual columns.  Returns (gap_k, sine / bound or None)."""
    assert E.shape == (n, k) and lam.shape == res.shape == (k,)
    assert res.max() <= tol and it < max_iter
    w, U = top_eigenpairs(M_host)
    assert np.all(np.abs(lam - w[:k]) <= res.max() + n * EPS), float(np.abs(lam - w[:k]).max())
    gap = float(w[k - 1] - w[k])
    assert (gap >= MIN_GAP) == subspace, gap
    if not subspace:
        return gap, None
    sine = SO.subspace_sine(SO.orthonormal(E, dd), U[:, :k])
    bound = np.sqrt(k) * res.max() / gap + n * EPS
    assert sine <= bound, (sine, bound)
    return gap, sine / bound
