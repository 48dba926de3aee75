"""Extended-precision restatement of one IncrementalPCA batch  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference of tests/test_ipca_hp_cpu.py and tests/test_gpu_ipca_edges.py: what frisk_amd/csrc/ipca_kernels.h computes for one
batch (statistics, stacked matrix A, G = AT A) and for a transform, in x87 extended precision (np.longdouble, 64-bit mantissa),
serially: column sums row by row, no splits, no tiles, no padding.  It shares no code with ipca_kernels.h or tests/ipca_oracle.py.

    batch(Xb, seen, mean, var, S, Vt, cols=None)   T, mean, var, A, G (all columns, or A[:, cols]T A) and the units below
    transform(X, mean, Vt)                          Y = (X - mean) VtT and its unit

Every compared quantity comes with a per-entry FORWARD-ERROR UNIT, built from long-double quantities only; a comparison is the
ratio |got - oracle| / unit (`ratio`).  With eps = 2^-52, b rows x, batch mean T, e = x - T, count = seen + b:

  rounding carried by an entry of A (dA)
        batch row        eps (|x| + |T|)                       (first batch: |mean_new| for |T|)
        head row i       eps |S_i Vt_ic|
        correction row   eps coef (|mean_old| + |T|),  coef = sqrt(seen / count * b)
  G_ij  eps sum_r |A_ri| |A_rj|  +  sum_r (|A_ri| dA_rj + dA_ri |A_rj| + dA_ri dA_rj)
  mean  eps (seen |mean_old| + sum_r |x|) / count
  var   [ eps (seen var_old + sum_r e^2 + (sum_r e)^2 / b + cross)  +  sum_r (2 |e| de + de^2)
          + seen / (b count) (2 |t| dt + dt^2) ] / count
        with de = eps (|x| + |T|) the uncertainty of every x - T, t = b mean_old - sum_r x the merge's difference of sums,
        dt = eps (b |mean_old| + sum_r |x|) and cross = seen / (b count) t^2 the merge's cross term
  Y_q   eps sum_c (|x_c| + |mean_c|) |V_cq|

The second-order terms (dA dA, de^2, dt^2) matter only where the first-order ones vanish: a constant column, whose e is zero in
exact arithmetic and a few 1e-17 in double.  A unit of exactly 0 (an all-zero column) demands got == oracle.

`distance_from_mp` (mpmath, 50 digits) measures this module's own distance from exact arithmetic in the same units; it is recorded
in tests/golden/ipca_hp.json for three small cases, one of them a later batch.
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, (
    "the IncrementalPCA reference needs an extended-precision long double (x87, 64-bit mantissa); this platform's has %d bits: "
    "the tests would silently compare double against double" % (np.finfo(np.longdouble).nmant + 1))

LD = np.longdouble
EPS = LD(2.0) ** -52


def _ld(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).astype(LD)


def _colsum(a):
    return np.add.reduce(a, axis=0)         # row by row (the reduced axis is the outer one): a serial sum per column


def batch(Xb, seen=0, mean=None, var=None, S=None, Vt=None, cols=None):
    """One batch from the state (seen, mean, var, S, Vt) (seen = 0: none).  A dict of long-double arrays: T, mean, var, A, G
    (f x f, or len(cols) x f = A[:, cols]T A), the units u_mean, u_var, u_G, and the shares `corr_share` (the correction row's
    part of trace G) and `cross_share` (the cross term's part of the summed variance)."""
    x = _ld(Xb)
    b, f = x.shape
    seen = int(seen)
    ax = np.abs(x)
    new_sum, abs_sum = _colsum(x), _colsum(ax)
    nb, count = LD(b), LD(seen + b)
    T = new_sum / nb
    e = x - T
    corr = _colsum(e)
    sq = _colsum(e * e)
    new_unnorm = sq - corr * corr / nb
    de = EPS * (ax + np.abs(T))
    prop = _colsum(LD(2) * np.abs(e) * de + de * de)
    out = {"T": T, "b": b, "seen": seen}
    if seen == 0:
        out["mean"] = new_sum / count
        out["var"] = new_unnorm / count
        out["u_mean"] = EPS * abs_sum / count
        out["u_var"] = (EPS * (sq + corr * corr / nb) + prop) / count
        A = x - out["mean"]
        dA = EPS * (ax + np.abs(out["mean"]))
        out["corr_share"] = out["cross_share"] = 0.0
    else:
        m0, v0, s0, vt0 = _ld(mean), _ld(var), _ld(S), _ld(Vt)
        ns = LD(seen)
        last_sum = m0 * ns
        over = ns / nb
        t = last_sum / over - new_sum
        cross = over / count * (t * t)
        out["mean"] = (last_sum + new_sum) / count
        out["var"] = (v0 * ns + new_unnorm + cross) / count
        out["u_mean"] = EPS * (np.abs(last_sum) + abs_sum) / count
        dt = EPS * (np.abs(last_sum) / over + abs_sum)
        out["u_var"] = (EPS * (np.abs(v0) * ns + sq + corr * corr / nb + cross) + prop
                        + over / count * (LD(2) * np.abs(t) * dt + dt * dt)) / count
        coef = np.sqrt(ns / count * nb)
        head = s0[:, None] * vt0
        last = coef * (m0 - T)
        A = np.vstack((head, e, last[None, :]))
        dA = np.vstack((EPS * np.abs(head), de, (EPS * coef * (np.abs(m0) + np.abs(T)))[None, :]))
        out["cross_share"] = float(np.sum(cross / count) / np.sum(out["var"])) if np.sum(out["var"]) > 0 else 0.0
    aA = np.abs(A)
    if cols is None:
        Ac, aAc, dAc = A, aA, dA
    else:
        cols = np.asarray(cols, dtype=np.int64)
        Ac, aAc, dAc = A[:, cols], aA[:, cols], dA[:, cols]
    out["A"] = A
    out["G"] = Ac.T @ A
    out["u_G"] = EPS * (aAc.T @ aA) + aAc.T @ dA + dAc.T @ (aA + dA)
    if seen:
        tr = np.sum(A * A)
        out["corr_share"] = float(np.sum(A[-1] * A[-1]) / tr) if tr > 0 else 0.0
    return out


def transform(X, mean, Vt):
    """(Y, u_Y) of Y = (X - mean) VtT; mean may be long double already (the oracle's own new mean)."""
    x = _ld(X)
    m = np.asarray(mean).astype(LD)
    v = _ld(Vt)
    return (x - m) @ v.T, EPS * ((np.abs(x) + np.abs(m)) @ np.abs(v).T)


def ratio(got, want, unit):
    """Worst |got - want| / unit over the entries; an entry whose unit is 0 must be equal (else inf)."""
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    unit = np.broadcast_to(unit, err.shape)
    pos = unit > 0
    r = np.where(pos, err / np.where(pos, unit, LD(1)), np.where(err == 0, LD(0), LD(np.inf)))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ mpmath
def _mp_of(v):
    """An exact mpmath value of a long double (or double)."""
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def distance_from_mp(Xb, seen=0, mean=None, var=None, S=None, Vt=None, Vt_new=None):
    """{G, mean, var, Y}: worst |this module - 50-digit arithmetic| / unit, for a small batch (python loops); Y is the transform
    of the batch itself with the new mean and Vt_new."""
    import mpmath as mp
    mp.mp.dps = 50
    o = batch(Xb, seen, mean, var, S, Vt)
    Xb = np.asarray(Xb, dtype=np.float64)
    b, f = Xb.shape
    x = [[mp.mpf(float(v)) for v in row] for row in Xb]
    new_sum = [mp.fsum(x[r][c] for r in range(b)) for c in range(f)]
    T = [s / b for s in new_sum]
    e = [[x[r][c] - T[c] for c in range(f)] for r in range(b)]
    unnorm = [mp.fsum(e[r][c] ** 2 for r in range(b)) - mp.fsum(e[r][c] for r in range(b)) ** 2 / b for c in range(f)]
    count = seen + b
    if seen == 0:
        mean_new = [s / count for s in new_sum]
        var_new = [u / count for u in unnorm]
        A = [[x[r][c] - mean_new[c] for c in range(f)] for r in range(b)]
    else:
        m0 = [mp.mpf(float(v)) for v in mean]
        v0 = [mp.mpf(float(v)) for v in var]
        mean_new = [(m0[c] * seen + new_sum[c]) / count for c in range(f)]
        over = mp.mpf(seen) / b
        var_new = [(v0[c] * seen + unnorm[c] + over / count * (m0[c] * seen / over - new_sum[c]) ** 2) / count for c in range(f)]
        coef = mp.sqrt(mp.mpf(seen) / count * b)
        A = [[mp.mpf(float(S[i])) * mp.mpf(float(Vt[i][c])) for c in range(f)] for i in range(len(S))]
        A += e
        A.append([coef * (m0[c] - T[c]) for c in range(f)])

    def worst(got, want, unit):
        w = mp.mpf(0)
        for g, t, u in zip(np.ravel(got), want, np.ravel(unit)):
            d = abs(_mp_of(g) - t)
            w = max(w, d / _mp_of(u)) if u > 0 else (w if d == 0 else mp.inf)
        return float(w)
    G = [mp.fsum(A[r][i] * A[r][j] for r in range(len(A))) for i in range(f) for j in range(f)]
    out = {"G": worst(o["G"], G, o["u_G"]), "mean": worst(o["mean"], mean_new, o["u_mean"]),
           "var": worst(o["var"], var_new, o["u_var"])}
    Y, uY = transform(Xb, o["mean"], Vt_new)
    Ymp = [mp.fsum((x[r][c] - mean_new[c]) * mp.mpf(float(Vt_new[q][c])) for c in range(f)) for r in range(b)
           for q in range(len(Vt_new))]
    out["Y"] = worst(Y, Ymp, uY)
    return out
