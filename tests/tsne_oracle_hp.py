"""Extended-precision restatement of exact t-SNE  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference of tests/test_tsne_hp_cpu.py and tests/test_gpu_tsne_edges.py: what frisk_amd/csrc/tsne_kernels.h computes (the
reference's x2p, symmetrise / normalise / clamp, and one iteration of its loop), with squared distances by direct differences,
in x87 extended precision (np.longdouble, 64-bit mantissa) and serially: every sum runs over its terms in index order, no tiles,
no butterflies.  It shares no code with tsne_kernels.h or tests/tsne_oracle.py.

    affinities(X, perplexity)                               beta, tries, q, the decision margins and the units below
    affinities(X, perplexity, beta=, total=, rel_total=, rows=, cols=)
                                                            q[rows][:, cols] and its unit from given betas (no bisection)
    step(Y, iY, gains, q, t, q_rel)                         dY, cost, gains, iY, Y after iteration t and the units below
    step(..., rows=, S=, rel_S=)                            dY, gains, iY of some rows from a given S (no centring)

The bisection evaluates H in long double, but carries beta / betamin / betamax in float64 as the reference and the kernel do:
where every decision (|Hdiff| > 1e-5, Hdiff > 0) agrees, beta is a dyadic path and equal bit for bit.  `m_tol` and `m_sign` are,
per row, the smallest | |Hdiff| - 1e-5 | and the smallest |Hdiff| over all tries: how far each decision was from flipping.

Every compared quantity comes with a per-entry FORWARD-ERROR UNIT, built from long-double quantities only, for an implementation
that takes DIRECT DIFFERENCES (there is no term for the cancellation of |a|^2 + |b|^2 - 2 a.b); a comparison is the ratio
|got - oracle| / unit (`ratio`).  With eps = 2^-52, f the width of X, d that of Y, and "rel" meaning relative to the value:

  e_ij = exp(-beta_i D_ij)   rel  g_ij = eps ((f + 2) beta_i D_ij + 1)       (f + 2 roundings carried by D, one by exp)
  sumP_i = sum_j e_ij        rel  r_i = eps + sum_j e_ij g_ij / sumP_i
  total = sum_ij p_j|i+p_i|j rel  rel_total = 3 eps + 2 sum_ij p_j|i (g_ij + r_i + eps) / total
  q_ij                       q_ij [ (p_j|i g_ij + p_i|j g_ji) / (p_j|i + p_i|j) + r_i + r_j + rel_total + 4 eps ]
                             (each conditional carries its own beta: at most eps (f + 2) (beta_i + beta_j) D_ij + eps, and only
                             beta_j's share where p_j|i underflows to 0, as in the rows that end on the upper beta cap)
                             (the clamp max(., fl(1e-12) / 4) is a contraction: the same unit holds on either side of it)
  H (for the record)         its margins are compared with 1e-9, four orders above eps (f + 2) beta D at the sizes used

  num_ij = 1 / (1 + D_ij)    rel  h_ij = eps ((d + 2) D_ij num_ij + 2)
  S = sum_ij num_ij          rel  rel_S = eps + sum_ij num_ij h_ij / S
  Q_ij = max(num / S, 1e-12) rel  h_ij + rel_S + eps
  coef_ij = (P - Q) num      u_coef = num (P q_rel + Q (h + rel_S + eps)) + |coef| (h + 2 eps)     (q_rel: the relative distance
                             between the q of the compared implementation and the q given here)
  dY_ik = sum_j coef_ij (y_ik - y_jk)
                             eps sum_j |coef_ij (y_ik - y_jk)| + sum_j (|y_ik - y_jk| u_coef_ij + 2 eps |coef_ij (y_ik - y_jk)|)
  cost = sum_ij P log(P / Q) eps sum |c_ij| + sum [ P q_rel (|log(P / Q)| + 1) + P (h + rel_S + 2 eps) + 2 eps |c_ij| ]
                             (diagonal included: num_ii = 0, so Q_ii = 1e-12)
  gains                      equal, unless |dY| <= (allowed ratio) x its unit: then the sign test is not decided
  iY_new = m iY - 500 g dY   500 g u_dY + eps (|m iY| + 1000 |g dY| + |iY_new|)
  pre = Y + iY_new           u_pre = u_iY + eps |pre|
  mean_k = sum_i pre_ik / n  u_mean = eps sum_i |pre_ik| / n + sum_i u_pre_ik / n + eps |mean_k|
  Y_new = pre - mean         u_pre + u_mean + eps |Y_new|

The gains (+ 0.2, x 0.8, the clamp at 0.01) are float64 arithmetic on float64 values and are carried in float64: they are
compared for equality.  A unit of exactly 0 demands got == oracle.

`distance_from_mp` (mpmath, 50 digits) measures this module's own distance from exact arithmetic in the same units; it is
recorded in tests/golden/tsne_hp.json for three small cases (affinities, an early step, a cost step).
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, (
    "the t-SNE reference needs an extended-precision long double (x87, 64-bit mantissa); this platform's has %d bits: "
    "the tests would silently compare double against double" % (np.finfo(np.longdouble).nmant + 1))

LD = np.longdouble
EPS = LD(2.0) ** -52
H_TOL = LD(1e-5)
MAX_TRIES = 50
Q_MIN = LD(1e-12)                   # fl(1e-12), the clamp of Q
Q_FLOOR = LD(1e-12) / LD(4)         # fl(1e-12) / 4, exact
STOP_EXAGGERATION, MOMENTUM_SWITCH = 100, 20
CHUNK = 256                         # rows handled at a time (memory only: every sum is serial along j)


def _ld(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).astype(LD)


def _rowsum(a):
    """Serial sum of every row in j order: the last column of the running sums, which numpy forms one term after another
    (its reductions sum pairwise along a contiguous axis, and a one-row block would be summed that way even when transposed)."""
    return np.add.accumulate(np.asarray(a, dtype=LD), axis=1)[:, -1]


def _sum(v):
    """Serial sum of a vector in index order."""
    return np.add.accumulate(np.asarray(v, dtype=LD))[-1] if len(v) else LD(0)


def _sqdist(A, rows, B=None):
    """(D, [differences per k]) of A[rows] against every row of B (default A): D = sum_k (a_ik - b_jk)^2 in k order."""
    B = A if B is None else B
    D = np.zeros((len(rows), B.shape[0]), dtype=LD)
    diffs = []
    for k in range(A.shape[1]):
        t = A[rows, k][:, None] - B[None, :, k]
        D += t * t
        diffs.append(t)
    return D, diffs


def _row_terms(x, beta, rows, f):
    """For the given rows: (e with a zero diagonal, sumP, r, D, g)."""
    D, _ = _sqdist(x, rows)
    b = beta[rows].astype(LD)[:, None]
    e = np.exp(-D * b)
    e[np.arange(len(rows)), rows] = 0
    g = EPS * ((f + 2) * b * D + 1)
    sumP = _rowsum(e)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = EPS + _rowsum(e * g) / sumP
    return e, sumP, r, D, g


def _bisect(x, rows, logU):
    """The reference's bisection for the given rows: beta (float64), tries, m_tol, m_sign."""
    m, n = len(rows), x.shape[0]
    D, _ = _sqdist(x, rows)
    off = np.ones((m, n), dtype=bool)
    off[np.arange(m), rows] = False

    def hdiff(idx, b):
        Di = D[idx]
        e = np.where(off[idx], np.exp(-Di * b.astype(LD)[:, None]), LD(0))
        s = _rowsum(e)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.log(s) + b.astype(LD) * _rowsum(Di * e) / s - logU

    beta = np.ones(m)
    bmin, bmax = np.full(m, -np.inf), np.full(m, np.inf)
    tries = np.zeros(m, dtype=np.int32)
    m_tol, m_sign = np.full(m, np.inf), np.full(m, np.inf)
    idx = np.arange(m)
    hd = hdiff(idx, beta)
    while True:
        a = np.abs(hd)
        with np.errstate(invalid="ignore"):
            m_tol[idx] = np.minimum(m_tol[idx], np.abs(a - H_TOL).astype(np.float64))
            m_sign[idx] = np.minimum(m_sign[idx], a.astype(np.float64))
            go = (a > H_TOL) & (tries[idx] < MAX_TRIES)          # a NaN stops the row, as in the reference
        idx, hd = idx[go], hd[go]
        if not len(idx):
            break
        up = hd > 0
        b = beta[idx]                                            # float64 from here, as the reference carries it
        lo, hi = bmin[idx], bmax[idx]
        lo = np.where(up, b, lo)
        hi = np.where(up, hi, b)
        with np.errstate(invalid="ignore"):
            nb = np.where(up, np.where(np.isinf(hi), b * 2.0, (b + hi) / 2.0), np.where(np.isinf(lo), b / 2.0, (b + lo) / 2.0))
        beta[idx], bmin[idx], bmax[idx] = nb, lo, hi
        tries[idx] += 1
        hd = hdiff(idx, nb)
    return beta, tries, m_tol, m_sign


def _totals(x, beta, f):
    """(sumP, r) of every row, total = sum_ij (p_j|i + p_i|j) as twice the serial sum of the conditionals, and rel_total."""
    n = x.shape[0]
    sumP, r = np.empty(n, dtype=LD), np.empty(n, dtype=LD)
    tot, u = LD(0), LD(0)
    for i0 in range(0, n, CHUNK):
        rr = np.arange(i0, min(n, i0 + CHUNK))
        e, sumP[rr], r[rr], _, g = _row_terms(x, beta, rr, f)
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = e / sumP[rr][:, None]
            tot = tot + _sum(_rowsum(cond))
            u = u + _sum(_rowsum(cond * (g + (r[rr] + EPS)[:, None])))
    return sumP, r, 2 * tot, 2 * EPS + (2 * u + EPS * 2 * tot) / (2 * tot)


def affinities(X, perplexity=None, beta=None, total=None, rel_total=None, rows=None, cols=None):
    """A dict.  Without beta: beta, tries, m_tol, m_sign, total, rel_total, and q, u_q (n x n, long double).  With beta (all
    rows'), total and rel_total: q and u_q for rows x cols only, without any bisection."""
    x = _ld(X)
    n, f = x.shape
    out = {}
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    cols = np.arange(n) if cols is None else np.asarray(cols, dtype=np.int64)
    if beta is None:
        logU = LD(np.log(np.float64(perplexity)))
        parts = [_bisect(x, np.arange(i0, min(n, i0 + CHUNK)), logU) for i0 in range(0, n, CHUNK)]
        beta, out["tries"], out["m_tol"], out["m_sign"] = [np.concatenate([p[k] for p in parts]) for k in range(4)]
        out["beta"] = beta
        sumP, r, total, rel_total = _totals(x, beta, f)
        out["total"], out["rel_total"] = total, rel_total
    else:
        beta = np.asarray(beta, dtype=np.float64)
        need = np.union1d(rows, cols)
        sumP, r = np.empty(n, dtype=LD), np.empty(n, dtype=LD)
        for i0 in range(0, len(need), CHUNK):
            rr = need[i0:i0 + CHUNK]
            _, sumP[rr], r[rr], _, _ = _row_terms(x, beta, rr, f)
    tot, rel_total = LD(total), LD(rel_total)
    D, _ = _sqdist(x, rows, x[cols])
    b = beta.astype(LD)
    same = rows[:, None] == cols[None, :]
    e_ij = np.where(same, LD(0), np.exp(-D * b[rows][:, None]))
    e_ji = np.where(same, LD(0), np.exp(-D * b[cols][None, :]))
    with np.errstate(divide="ignore", invalid="ignore"):
        sym = e_ij / sumP[rows][:, None] + e_ji / sumP[cols][None, :]
        out["q"] = np.maximum(sym / tot, Q_FLOOR)
        a, c = e_ij / sumP[rows][:, None], e_ji / sumP[cols][None, :]
        g = (a * (EPS * ((f + 2) * b[rows][:, None] * D + 1)) + c * (EPS * ((f + 2) * b[cols][None, :] * D + 1)))
        g = np.where(sym > 0, g / np.where(sym > 0, sym, LD(1)), LD(0))
        out["u_q"] = out["q"] * (g + r[rows][:, None] + r[cols][None, :] + rel_total + 4 * EPS)
        out["below_floor"] = (sym / tot < Q_FLOOR / 2) & ~same      # not within any unit of the clamp: q is the floor, exactly
    return out


def step(Y, iY, gains, q, t, q_rel=0.0, rows=None, S=None, rel_S=None):
    """Iteration t of the reference's loop from (Y, iY, gains), float64 arrays, with q (n x n, or rows x n with rows) as the
    normalised clamped affinities.  A dict of dY, gains (float64), iY, Y, cost (None unless (t + 1) % 10 == 0), S, rel_S, Q_clamped
    (the share of off-diagonal pairs whose Q is at the clamp) and the units u_dY, u_iY, u_Y, u_cost.  With rows: those rows of dY,
    gains and iY only, from the given S and rel_S; no Y and no cost."""
    y, iy = _ld(Y), _ld(iY)
    n, d = y.shape
    sub = rows is not None
    rows = np.asarray(rows, dtype=np.int64) if sub else np.arange(n)
    q = np.asarray(q, dtype=LD)
    q_rel = LD(q_rel)
    if not sub:
        S_acc, hs_acc = LD(0), LD(0)
        for i0 in range(0, n, CHUNK):
            rr = np.arange(i0, min(n, i0 + CHUNK))
            D, _ = _sqdist(y, rr)
            num = 1 / (1 + D)
            num[np.arange(len(rr)), rr] = 0
            S_acc = S_acc + _sum(_rowsum(num))
            hs_acc = hs_acc + _sum(_rowsum(num * (EPS * ((d + 2) * D * num + 2))))
        S, rel_S = S_acc, EPS + hs_acc / S_acc
    S, rel_S = LD(S), LD(rel_S)
    m = len(rows)
    dY, u_dY = np.empty((m, d), dtype=LD), np.empty((m, d), dtype=LD)
    cost, u_cost, clamped = LD(0), LD(0), 0
    with_cost = (t + 1) % 10 == 0 and not sub
    for i0 in range(0, m, CHUNK):
        sl = slice(i0, min(m, i0 + CHUNK))
        rr = rows[sl]
        D, diffs = _sqdist(y, rr)
        num = 1 / (1 + D)
        num[np.arange(len(rr)), rr] = 0
        h = EPS * ((d + 2) * D * num + 2)
        Q = np.maximum(num / S, Q_MIN)
        P = q[sl] * 4 if t <= STOP_EXAGGERATION else q[sl]
        coef = (P - Q) * num
        u_coef = num * (P * q_rel + Q * (h + rel_S + EPS)) + np.abs(coef) * (h + 2 * EPS)
        for k in range(d):
            term = coef * diffs[k]
            at = np.abs(term)
            dY[sl, k] = _rowsum(term)
            u_dY[sl, k] = EPS * _rowsum(at) + _rowsum(np.abs(diffs[k]) * u_coef + 2 * EPS * at)
        off = num > 0
        clamped += int(np.count_nonzero((Q == Q_MIN) & off))
        if with_cost:
            lg = np.log(P / Q)
            c = P * lg
            cost = cost + _sum(_rowsum(c))
            u_cost = u_cost + _sum(_rowsum(EPS * np.abs(c) + P * q_rel * (np.abs(lg) + 1) + P * (h + rel_S + 2 * EPS)
                                                    + 2 * EPS * np.abs(c)))
    g0 = np.asarray(gains, dtype=np.float64)[rows]
    flip = (dY > 0) != (iy[rows] > 0)
    g = np.where(flip, g0 + 0.2, g0 * 0.8)                  # float64, as the reference and the kernel carry the gains
    g[g < 0.01] = 0.01
    mom = LD(0.5) if t < MOMENTUM_SWITCH else LD(0.8)       # fl(0.8), the constant both implementations multiply by
    gd = g.astype(LD) * dY
    niy = mom * iy[rows] - 500 * gd
    u_iY = 500 * g.astype(LD) * u_dY + EPS * (np.abs(mom * iy[rows]) + 1000 * np.abs(gd) + np.abs(niy))
    out = {"dY": dY, "u_dY": u_dY, "gains": g, "iY": niy, "u_iY": u_iY, "S": S, "rel_S": rel_S,
           "Q_clamped": clamped / float(max(1, m * (n - 1))), "cost": None, "u_cost": None}
    if sub:
        return out
    pre = y + niy
    u_pre = u_iY + EPS * np.abs(pre)
    mean = _rowsum(pre.T) / n               # column sums, row after row
    u_mean = EPS * _rowsum(np.abs(pre).T) / n + _rowsum(u_pre.T) / n + EPS * np.abs(mean)
    out["Y"] = pre - mean
    out["u_Y"] = u_pre + u_mean + EPS * np.abs(out["Y"])
    if with_cost:
        out["cost"], out["u_cost"] = cost, u_cost
    return out


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


def distance_from_mp(X=None, perplexity=None, Y=None, iY=None, gains=None, q=None, t=None):
    """Worst |this module - 50-digit arithmetic| / unit for a small case (python loops).  With X: {q} from this module's own
    betas.  With Y: {dY, iY, Y, cost (cost iterations only)} of step(Y, iY, gains, q, t) with q float64."""
    import mpmath as mp
    mp.mp.dps = 50
    if X is not None:
        o = affinities(X, perplexity)
        X = np.asarray(X, dtype=np.float64)
        n, f = X.shape
        x = [[mp.mpf(float(v)) for v in row] for row in X]
        b = [mp.mpf(float(v)) for v in o["beta"]]
        D = [[mp.fsum((x[i][k] - x[j][k]) ** 2 for k in range(f)) for j in range(n)] for i in range(n)]
        e = [[mp.exp(-D[i][j] * b[i]) if i != j else mp.mpf(0) for j in range(n)] for i in range(n)]
        s = [mp.fsum(row) for row in e]
        sym = [[e[i][j] / s[i] + e[j][i] / s[j] for j in range(n)] for i in range(n)]
        tot = mp.fsum(mp.fsum(row) for row in sym)
        floor = _mp_of(Q_FLOOR)
        qq = [max(sym[i][j] / tot, floor) for i in range(n) for j in range(n)]
        return {"q": _mp_worst(o["q"], qq, o["u_q"])}
    o = step(Y, iY, gains, q, t)
    Y, iY, q = (np.asarray(a, dtype=np.float64) for a in (Y, iY, q))
    n, d = Y.shape
    y = [[mp.mpf(float(v)) for v in row] for row in Y]
    num = [[1 / (1 + mp.fsum((y[i][k] - y[j][k]) ** 2 for k in range(d))) if i != j else mp.mpf(0) for j in range(n)]
           for i in range(n)]
    S = mp.fsum(mp.fsum(row) for row in num)
    qmin = _mp_of(Q_MIN)
    Q = [[max(num[i][j] / S, qmin) for j in range(n)] for i in range(n)]
    P = [[mp.mpf(float(q[i][j])) * (4 if t <= STOP_EXAGGERATION else 1) for j in range(n)] for i in range(n)]
    dY = [[mp.fsum((P[i][j] - Q[i][j]) * num[i][j] * (y[i][k] - y[j][k]) for j in range(n)) for k in range(d)] for i in range(n)]
    mom = mp.mpf(0.5 if t < MOMENTUM_SWITCH else 0.8)
    niy = [[mom * mp.mpf(float(iY[i][k])) - 500 * mp.mpf(float(o["gains"][i][k])) * dY[i][k] for k in range(d)] for i in range(n)]
    pre = [[y[i][k] + niy[i][k] for k in range(d)] for i in range(n)]
    mean = [mp.fsum(pre[i][k] for i in range(n)) / n for k in range(d)]
    out = {"dY": _mp_worst(o["dY"], [v for row in dY for v in row], o["u_dY"]),
           "iY": _mp_worst(o["iY"], [v for row in niy for v in row], o["u_iY"]),
           "Y": _mp_worst(o["Y"], [pre[i][k] - mean[k] for i in range(n) for k in range(d)], o["u_Y"])}
    if o["cost"] is not None:
        c = mp.fsum(P[i][j] * mp.log(P[i][j] / Q[i][j]) for i in range(n) for j in range(n))
        out["cost"] = float(abs(_mp_of(o["cost"]) - c) / _mp_of(o["u_cost"]))
    return out
