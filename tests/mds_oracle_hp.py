"""Extended-precision restatement of metric MDS  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference of tests/test_mds_hp_cpu.py and tests/test_gpu_mds_edges.py: what frisk_amd/csrc/mds_kernels.h computes (the
dissimilarities, one SMACOF pass, and the loop of State::run, which is sklearn 1.7's _smacof_single with metric=True), with
every distance by direct differences, in x87 extended precision (np.longdouble, 64-bit mantissa) and serially: every sum runs
over its terms in index order, no tiles, no butterflies.  It shares no code with mds_kernels.h or tests/mds_oracle.py.

    dissimilarities(X, rows=None)       D[rows] = sqrt(sum_k (x_ik - x_jk)^2), k in order, and its unit
    step(Y, D, rows=None)               for float64 Y and D: Y1[rows] = (1 / n) sum_{j != i} ratio_ij (y_i - y_j) with
                                        ratio_ij = D_ij / (dist_ij == 0 ? 1e-5 : dist_ij); stress = sum_ij (dist_ij - D_ij)^2 / 2
                                        and sumsq = sum_ij dist_ij^2 of the configuration Y itself; their units
    run(Y0, D, max_iter, eps)           the driver: one Guttman pass whose stress is unused, then per iteration it the stress
                                        of X_{it+1}, stopping when it > 0 and v_it = (old - stress) / (sumsq / 2) < eps, and no
                                        Guttman update on the last pass; the states X_1 .., the trace, v_it, n_iter

Every compared quantity comes with a per-entry FORWARD-ERROR UNIT, built from long-double quantities only, for an implementation
that takes DIRECT DIFFERENCES: there is no term for the cancellation of |a|^2 + |b|^2 - 2 a.b, and nothing depends on |x| or
|y|, so a uniform shift of the input leaves every unit unchanged (tests/test_mds_hp_cpu.py asserts it).  A comparison is the
ratio |got - oracle| / unit (`ratio`).  With eps = 2^-52, f the width of X, d that of Y, "rel" meaning relative to the value:

  D_ij                       rel  eps ((f + 2) / 2 + 1)
                             (each (x_ik - x_jk)^2 carries 3 roundings, two from the difference that is squared and one from
                             the product, and the sum f - 1 more: f + 2 on the squared distance, halved by the root, which
                             adds one of its own)
  dist_ij                    rel  h = eps ((d + 2) / 2 + 1)                              (the same, over d columns)
  term_ijk = ratio_ij (y_ik - y_jk)
                             rel  h + 3 eps     (the quotient D_ij / dist_ij carries h and its own rounding, the difference one,
                             the product one; a pair with dist_ij == 0 has y_i == y_j and a term of exactly 0 on either side
                             of the zero rule, as long as the replaced quotient is finite)
  Y1_ik                      [ sum_j |term_ijk| (h + 3 eps) + eps sum_j |term_ijk| ] / n + eps |Y1_ik|
                             (the terms' own errors, the sum's roundings at one eps of the absolute sum, the scaling by 1 / n)
  e_ij = dist_ij - D_ij      abs  u_e = h dist_ij + eps |e_ij|                           (D is given: only dist carries error)
  stress                     (1 / 2) sum_ij (2 |e_ij| u_e + u_e^2 + 2 eps e_ij^2)
                             ((e + u)^2 - e^2, then the square's rounding and the sum's at one eps each of the absolute sum)
  sumsq                      rel  2 h + 2 eps
  X_{t+1} of run             u_{t+1,ik} = unit of Y1_ik at X_t + (1 / n) sum_j ratio_ij (|u_t,i| + |u_t,j|), |u_t,i| the
                             Euclidean norm of row i of the unit of X_t (u_0 = 0): the derivative of ratio_ij (y_i - y_j) by
                             y_i - y_j is ratio_ij (I - w w^T), w the unit vector of the difference, of norm ratio_ij

A unit of exactly 0 demands got == oracle: D on the diagonal and between duplicate rows, and Y1 of an all-coincident
configuration, which is exactly 0.  The constant 1e-5 is the double nearest to it, as the kernel and sklearn carry it.

`distance_from_mp` (mpmath, 50 digits) measures this module's own distance from exact arithmetic in the same units; it is
recorded in tests/golden/mds_hp.json for three small cases (one D, one step, one stress).
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, (
    "the MDS reference needs an extended-precision long double (x87, 64-bit mantissa); this platform's has %d bits: "
    "the tests would silently compare double against double" % (np.finfo(np.longdouble).nmant + 1))

LD = np.longdouble
EPS = LD(2.0) ** -52
ZERO_DIST = LD(np.float64(1e-5))    # fl(1e-5)
CHUNK = 256                         # rows handled at a time (memory only: every sum is serial along j)


def _ld(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).astype(LD)


def _rowsum(a):
    """Serial sum of every row in j order: the last column of the running sums, which numpy forms one term after another
    (its reductions sum pairwise along a contiguous axis)."""
    return np.add.accumulate(a, axis=1)[:, -1]


def _sum(v):
    """Serial sum of a vector in index order."""
    return np.add.accumulate(v)[-1] if len(v) else LD(0)


def _dist(a, rows, keep=True):
    """(dist, [differences per k]) of a[rows] against every row of a: sqrt(sum_k (a_ik - a_jk)^2), k in order; in a's type."""
    s = np.zeros((len(rows), a.shape[0]), dtype=a.dtype)
    diffs = []
    for k in range(a.shape[1]):
        t = a[rows, k][:, None] - a[None, :, k]
        s += t * t
        if keep:
            diffs.append(t)
    return np.sqrt(s), diffs


def _chunks(rows):
    return [(slice(i0, min(len(rows), i0 + CHUNK)), rows[i0:i0 + CHUNK]) for i0 in range(0, len(rows), CHUNK)]


def h_of(d):
    return EPS * (LD(d + 2) / 2 + 1)


def dissimilarities(X, rows=None):
    """(D[rows], its unit), long double; all rows by default."""
    x = _ld(X)
    n, f = x.shape
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    D = np.empty((len(rows), n), dtype=LD)
    for sl, rr in _chunks(rows):
        D[sl] = _dist(x, rr, keep=False)[0]
    D[np.arange(len(rows)), rows] = 0
    return D, D * h_of(f)


def _guttman(y, D, rows, units=True, spread=None):
    """(Y1[rows], unit) from the configuration y and dissimilarities D, both of one type (long double for the oracle; float64,
    without units, where a test only needs a deterministic input).  spread: |u_i| per row of y, for run's propagated unit."""
    n, d = y.shape
    Y1 = np.empty((len(rows), d), dtype=y.dtype)
    U = np.zeros((len(rows), d), dtype=LD) if units else None
    h = h_of(d)
    zero = y.dtype.type(ZERO_DIST)
    for sl, rr in _chunks(rows):
        dist, diffs = _dist(y, rr)
        ratio = D[rr] / np.where(dist == 0, zero, dist)
        ratio[np.arange(len(rr)), rr] = 0
        for k in range(d):
            term = ratio * diffs[k]
            Y1[sl, k] = _rowsum(term) / n
            if units:
                sa = _rowsum(np.abs(term))
                U[sl, k] = (sa * (h + 3 * EPS) + EPS * sa) / n + EPS * np.abs(Y1[sl, k])
        if units and spread is not None:
            U[sl] += (_rowsum(ratio * (spread[rr][:, None] + spread[None, :])) / n)[:, None]
    return Y1, U


def _sums(y, D):
    """(stress, its unit, sumsq, its unit) of the configuration y (long double)."""
    n, d = y.shape
    h = h_of(d)
    st, u, sq = LD(0), LD(0), LD(0)
    for _sl, rr in _chunks(np.arange(n)):
        dist, _ = _dist(y, rr, keep=False)
        e = dist - D[rr]
        ae = np.abs(e)
        ue = h * dist + EPS * ae
        st = st + _sum(_rowsum(e * e))
        u = u + _sum(_rowsum(2 * ae * ue + ue * ue + 2 * EPS * e * e))
        sq = sq + _sum(_rowsum(dist * dist))
    return st / 2, u / 2, sq, sq * (2 * h + 2 * EPS)


def step(Y, D, rows=None, guttman=True, sums=True):
    """A dict for float64 Y (n x d) and D (n x n).  With guttman: Y1, u_Y1 (rows x d; all rows by default).  With sums: stress,
    u_stress, sumsq, u_sumsq of Y itself."""
    y, Dl = _ld(Y), _ld(D)
    n = y.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    out = {}
    if guttman:
        out["Y1"], out["u_Y1"] = _guttman(y, Dl, rows)
    if sums:
        out["stress"], out["u_stress"], out["sumsq"], out["u_sumsq"] = _sums(y, Dl)
    return out


def run(Y0, D, max_iter, eps):
    """The loop of State::run in long double from the float64 start Y0.  A dict: states (X_1 .. X_{n_iter}, the last one is the
    result), u_states, trace (the stress of X_{it+1} per iteration), sumsq, v (v[0] is NaN), n_iter."""
    Dl = _ld(D)
    n = Dl.shape[0]
    rows = np.arange(n)
    cur, u = _guttman(_ld(Y0), Dl, rows)
    states, units, trace, sumsqs, vs = [cur], [u], [], [], []
    old, it = LD(0), 0
    while True:
        last = it + 1 >= max_iter
        stress, _us, sq, _uq = _sums(cur, Dl)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (old - stress) / (sq / 2) if it > 0 else LD(np.nan)
        trace.append(stress)
        sumsqs.append(sq)
        vs.append(v)
        if it > 0 and v < eps:
            break
        old = stress
        if last:
            break
        cur, u = _guttman(cur, Dl, rows, spread=np.sqrt(_rowsum(u * u)))
        states.append(cur)
        units.append(u)
        it += 1
    return {"states": states, "u_states": units, "trace": trace, "sumsq": sumsqs, "v": vs, "n_iter": it + 1}


def settle(Y, D, steps):
    """`steps` Guttman updates from Y carried in float64 with this module's serial sums: only + - * / sqrt in a fixed order, so
    the result is the same bit for bit everywhere.  It makes inputs, not references."""
    y = np.ascontiguousarray(Y, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    rows = np.arange(y.shape[0])
    for _ in range(steps):
        y = _guttman(y, D, rows, units=False)[0]
    return y


def ratio(got, want, unit, where=None):
    """Worst |got - want| / unit over the entries (those of the mask `where`); an entry whose unit is 0 must be equal (else inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    unit = np.broadcast_to(unit, err.shape)
    pos = unit > 0
    r = np.where(pos, err / np.where(pos, unit, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    if where is not None:
        r = r[where]
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ mpmath
def _mp_of(v):
    """An exact mpmath value of a long double (or double)."""
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def _mp_worst(got, want, unit):
    import mpmath as mp
    w = mp.mpf(0)
    for g, t, u in zip(np.ravel(got), want, np.ravel(unit)):
        dlt = abs(_mp_of(g) - t)
        w = max(w, dlt / _mp_of(u)) if u > 0 else (w if dlt == 0 else mp.inf)
    return float(w)


def distance_from_mp(X=None, Y=None, D=None):
    """Worst |this module - 50-digit arithmetic| / unit for a small case (python loops).  With X: {D}.  With Y and D (float64):
    {Y1, stress, sumsq} of step(Y, D)."""
    import mpmath as mp
    mp.mp.dps = 50
    if X is not None:
        got, unit = dissimilarities(X)
        X = np.asarray(X, dtype=np.float64)
        n, f = X.shape
        x = [[mp.mpf(float(v)) for v in row] for row in X]
        want = [mp.sqrt(mp.fsum((x[i][k] - x[j][k]) ** 2 for k in range(f))) for i in range(n) for j in range(n)]
        return {"D": _mp_worst(got, want, unit)}
    o = step(Y, D)
    Y, D = np.asarray(Y, dtype=np.float64), np.asarray(D, dtype=np.float64)
    n, d = Y.shape
    y = [[mp.mpf(float(v)) for v in row] for row in Y]
    Dm = [[mp.mpf(float(v)) for v in row] for row in D]
    dist = [[mp.sqrt(mp.fsum((y[i][k] - y[j][k]) ** 2 for k in range(d))) for j in range(n)] for i in range(n)]
    zero = mp.mpf(float(ZERO_DIST))
    rat = [[Dm[i][j] / (zero if dist[i][j] == 0 else dist[i][j]) if i != j else mp.mpf(0) for j in range(n)] for i in range(n)]
    Y1 = [mp.fsum(rat[i][j] * (y[i][k] - y[j][k]) for j in range(n)) / n for i in range(n) for k in range(d)]
    stress = mp.fsum((dist[i][j] - Dm[i][j]) ** 2 for i in range(n) for j in range(n)) / 2
    sumsq = mp.fsum(dist[i][j] ** 2 for i in range(n) for j in range(n))
    return {"Y1": _mp_worst(o["Y1"], Y1, o["u_Y1"]), "stress": _mp_worst([o["stress"]], [stress], [o["u_stress"]]),
            "sumsq": _mp_worst([o["sumsq"]], [sumsq], [o["u_sumsq"]])}
