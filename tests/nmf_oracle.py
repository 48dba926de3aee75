"""sklearn 1.7's NMF(init=None, solver='cd', shuffle=False) restated in numpy for the tests, independently of frisk_amd.projection:
the start (_initialize_nmf: _randomized_svd + the NNDSVD split, or the 'random' draw), one iteration of _fit_coordinate_descent
(_update_cdnmf_fast with the identity permutation), the stop rule, and transform (W from zeros, H fixed).  No sklearn import.

Products.  `product(A, B, how)` is A @ B three ways: "blas" (numpy's matmul, what sklearn calls), "pairwise" (every entry summed
along a contiguous axis by numpy's pairwise add.reduce: a second honest double implementation with another summation order) and
"ld" (long double).  A sum of k products of doubles computed in any order, with or without fused multiply-add, lies within
gamma(k) sum |a_i b_i| of the exact value, gamma(k) = k eps / (1 - k eps) (Higham, Accuracy and Stability, section 3.1).

One step's forward-error bound (step_bound), to first order, for ONE double implementation against exact arithmetic from the same
input state (W, H):
  Gram      |dG[t][r]| <= gamma(m) sum_i |A_it A_ir|, plus the propagated input error sum_i (dA_it |A_ir| + |A_it| dA_ir);
  product   |dP[s][t]| <= gamma(m) (|X| |A|)[s][t], plus |X| dA;
  sweep     per row, t = 0 .. d - 1 in order, with dw_r the bound of the entries already updated in this sweep (0 for the others:
            the input is the same on both sides):
              |dg| <= dP[s][t] + sum_r (dG[t][r] |w_r| + |G[t][r]| dw_r) + gamma(d + 1) (|P[s][t]| + sum_r |G[t][r] w_r|)
              w' = max(w - g / G[t][t], 0): max(., 0) is 1-Lipschitz, so
              |dw_t| <= |dg| / |G[t][t]| + |g| dG[t][t] / G[t][t]^2 + eps |g / G[t][t]| + eps |w - g / G[t][t]|
            The branch W[s][t] == 0 is decided by the input state, identical on both sides; min(0, g) and |.| are 1-Lipschitz, so
              |d violation| <= sum |dg| + gamma(m d) violation.
  H sweep   the same on (HT, WT W, XT W), with dA = dW of the W sweep entering the Gram matrix and the product.
Two double implementations (the device and sklearn) each lie within that bound of the exact step, so their difference is within
twice it: step_bound(..., sides=2), the default.  Nothing in it is calibrated on measured values.
"""
import json
import os

import numpy as np

EPS = np.finfo(np.float64).eps
TOL, MAX_ITER, OVERSAMPLES, INIT_EPS = 1e-4, 200, 10, 1e-6
LD = np.longdouble

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(table="nmf"):
    """tests/golden/nmf.json, or with table = "nmf_edges" the second table (tools/make_golden_nmf.py --edges)."""
    return json.load(open(os.path.join(GOLD, table + ".json")))


def arrays(g, case):
    return np.load(os.path.join(GOLD, g.get("dir", "nmf"), g["cases"][case]["file"]))


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def make_X(spec):
    """Dirichlet-multinomial rows as tools/make_golden_nmf.py draws them (legacy RandomState streams are frozen): per block of
    `orders` a Dirichlet centre, per row a Dirichlet around it and a multinomial of `depth` draws, turned into proportions.
    Optional fields of the second table: "distinct" (only that many rows are drawn; the n rows are then picked among them, each
    at least once), "rank1" (the rows are the concatenated centres times a factor in [0.5, 1.5) each: an outer product), "absent"
    ({"cols": [...], "rows": [...]}, set to zero at the end: k-mers no window contains, and an empty row)."""
    rs = np.random.RandomState(spec["seed"])
    centre = [rs.dirichlet(np.full(w, 2.0)) for w in spec["orders"]]
    rows = []
    for _ in range(spec.get("distinct", 0 if spec.get("rank1") else spec["n"])):
        parts = []
        for c in centre:
            pr = rs.dirichlet(c * spec["spread"] + 1e-3)
            k = rs.multinomial(spec["depth"], pr)
            parts.append(k / float(k.sum()))
        rows.append(np.concatenate(parts))
    X = np.array(rows)
    if "distinct" in spec:
        m = spec["distinct"]
        X = X[np.concatenate([np.arange(m), rs.randint(m, size=spec["n"] - m)])[rs.permutation(spec["n"])]]
    if spec.get("rank1"):
        X = (0.5 + rs.random_sample(spec["n"]))[:, None] * np.concatenate(centre)[None, :]
    if "absent" in spec:
        X[:, spec["absent"]["cols"]] = 0.0
        X[spec["absent"]["rows"], :] = 0.0
    return X


# ------------------------------------------------------------------------------------------------ products
def product(A, B, how="blas"):
    if how == "blas":
        return A @ B
    if how == "ld":
        return np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD)
    if how == "pairwise":
        Bt = np.ascontiguousarray(B.T)
        return np.add.reduce(np.ascontiguousarray(A)[:, None, :] * Bt[None, :, :], axis=2)
    raise ValueError(how)


# ------------------------------------------------------------------------------------------------ the start
def svd_flip(U, Vt, u_based):
    if u_based:
        signs = np.sign(U[np.argmax(np.abs(U), axis=0), np.arange(U.shape[1])])
    else:
        signs = np.sign(Vt[np.arange(Vt.shape[0]), np.argmax(np.abs(Vt), axis=1)])
    return U * signs[None, :], Vt * signs[:, None]


def randomized_svd(X, d, seed, how="blas"):
    """_randomized_svd(X, d, random_state=seed) with the defaults NMF uses: (U n x d, S, V d x f)."""
    from scipy import linalg
    n, f = X.shape
    n_iter = 7 if d < 0.1 * min(n, f) else 4
    transpose = n < f
    M = X.T if transpose else X
    Q = np.random.RandomState(seed).normal(size=(M.shape[1], d + OVERSAMPLES))
    for _ in range(n_iter):
        Q, _ = linalg.lu(product(M, Q, how), permute_l=True, check_finite=False)
        Q, _ = linalg.lu(product(M.T, Q, how), permute_l=True, check_finite=False)
    Q, _ = linalg.qr(product(M, Q, how), mode="economic", check_finite=False)
    B = Q.T @ M if how == "blas" else product(M.T, Q, how).T
    Uhat, s, Vt = linalg.svd(B, full_matrices=False, lapack_driver="gesdd")
    U = Q @ Uhat
    U, Vt = svd_flip(U, Vt, not transpose)
    if transpose:
        return Vt[:d].T, s[:d], U[:, :d].T
    return U[:, :d], s[:d], Vt[:d]


def nndsvd_raw(U, S, V):
    """The NNDSVD split before the 1e-6 cut: (W, H, [(m_p, m_n) of the columns 1 .. d - 1])."""
    W, H, ms = np.zeros_like(U), np.zeros_like(V), []
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(V[0, :])
    for j in range(1, U.shape[1]):
        x, y = U[:, j], V[j, :]
        xp, yp = np.maximum(x, 0), np.maximum(y, 0)
        xn, yn = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        xpn, ypn, xnn, ynn = (np.sqrt(np.dot(v, v)) for v in (xp, yp, xn, yn))
        m_p, m_n = xpn * ypn, xnn * ynn
        ms.append((float(m_p), float(m_n)))
        if m_p > m_n:
            u, v, sigma = xp / xpn, yp / ypn, m_p
        else:
            u, v, sigma = xn / xnn, yn / ynn, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j] = lbd * u
        H[j, :] = lbd * v
    return W, H, ms


def initialize(X, d, seed, how="blas"):
    """_initialize_nmf(X, d, init=None, random_state=seed): (W0, H0)."""
    n, f = X.shape
    if d > min(n, f):
        avg = np.sqrt(X.mean() / d)
        rs = np.random.RandomState(seed)
        H = avg * rs.standard_normal(size=(d, f))
        W = avg * rs.standard_normal(size=(n, d))
        return np.abs(W), np.abs(H)
    W, H, _ = nndsvd_raw(*randomized_svd(X, d, seed, how))
    avg = X.mean()
    for A in (W, H):
        A[A < INIT_EPS] = 0
        A[A == 0] = avg
    return W, H


# ------------------------------------------------------------------------------------------------ one step
def sweep(W, G, P, eG=None, eP=None, pre=None, grad=None):
    """_update_cdnmf_fast(W, HHt = G, XHt = P, identity) on a copy, every row at once, in the dtype of the inputs.  Returns
    (W', violation) or, with the input bounds eG and eP, (W', violation, dW bound, violation bound).  pre, an m x d array, receives every entry before its max(., 0)
    (columns with a zero Hessian are left as they come); grad, m x d, every entry's gradient g."""
    W = W.copy()
    m, d = W.shape
    bound = eG is not None
    viol = W.dtype.type(0)
    dW, ev = np.zeros((m, d)), 0.0
    for t in range(d):
        g = -P[:, t]
        for r in range(d):
            g = g + G[t, r] * W[:, r]
        pg = np.where(W[:, t] == 0, np.minimum(0, g), g)
        viol = viol + np.abs(pg).sum()
        if grad is not None:
            grad[:, t] = g
        if bound:
            aW = np.abs(W).astype(np.float64)
            aG = np.abs(G[t]).astype(np.float64)
            mag = np.abs(P[:, t]).astype(np.float64) + (aG[None, :] * aW).sum(axis=1)
            eg = eP[:, t] + (eG[t][None, :] * aW).sum(axis=1) + (aG[None, :] * dW).sum(axis=1) + gamma(d + 1) * mag
            ev += float(eg.sum())
        if G[t, t] != 0:
            q = g / G[t, t]
            v = W[:, t] - q
            if bound:
                h = float(abs(G[t, t]))
                dW[:, t] = eg / h + np.abs(g).astype(np.float64) * eG[t, t] / (h * h) + EPS * np.abs(q) + EPS * np.abs(v)
            if pre is not None:
                pre[:, t] = v
            W[:, t] = np.maximum(v, 0)
    if bound:
        return W, viol, dW, ev + gamma(m * d) * float(viol)
    return W, viol


def step(X, W, H, update_H=True, how="blas", aux=None):
    """One iteration of _fit_coordinate_descent from (W, H): (W', H', violation).  how = "ld" computes everything in long
    double and returns long doubles.  aux, a dict, receives sweep's pre and grad of the W sweep ("preW", "gradW", n x d, pre
    starting from W) and, with update_H, of the H sweep ("preH", "gradH", d x f)."""
    if how == "ld":
        X, W, H = (np.asarray(a, dtype=LD) for a in (X, W, H))
    Ht = np.ascontiguousarray(H.T)
    pre, grad = (W.copy(), np.zeros_like(W)) if aux is not None else (None, None)
    W1, v = sweep(W, product(Ht.T, Ht, how), product(X, Ht, how), pre=pre, grad=grad)
    if aux is not None:
        aux.update(preW=pre, gradW=grad)
    if not update_H:
        return W1, H.copy(), v
    pre, grad = (Ht.copy(), np.zeros_like(Ht)) if aux is not None else (None, None)
    Ht1, v2 = sweep(Ht, product(W1.T, W1, how), product(X.T, W1, how), pre=pre, grad=grad)
    if aux is not None:
        aux.update(preH=np.ascontiguousarray(pre.T), gradH=np.ascontiguousarray(grad.T))
    return W1, np.ascontiguousarray(Ht1.T), v + v2


def step_bound(X, W, H, update_H=True, sides=2):
    """First-order forward-error bounds of one step from (W, H) (module docstring): (bW n x d, bH d x f, b_violation), each the
    bound for `sides` double implementations apart (1: one implementation against exact arithmetic)."""
    X, W, H = (np.asarray(a, dtype=np.float64) for a in (X, W, H))
    n, f = X.shape
    Ht = np.ascontiguousarray(H.T)
    aX, aHt = np.abs(X), np.abs(Ht)
    eG = gamma(f) * (aHt.T @ aHt)
    eP = gamma(f) * (aX @ aHt)
    W1, _v, dW, ev = sweep(W, Ht.T @ Ht, X @ Ht, eG, eP)
    if not update_H:
        return sides * dW, np.zeros_like(H), sides * ev
    aW = np.abs(W1)
    eG2 = gamma(n) * (aW.T @ aW) + dW.T @ aW + aW.T @ dW
    eP2 = gamma(n) * (aX.T @ aW) + aX.T @ dW
    _Ht1, _v2, dHt, ev2 = sweep(Ht, W1.T @ W1, X.T @ W1, eG2, eP2)
    return sides * dW, sides * np.ascontiguousarray(dHt.T), sides * (ev + ev2)


# ------------------------------------------------------------------------------------------------ whole runs
def iterate(X, W, H, update_H, tol=TOL, max_iter=MAX_ITER, how="blas", trace=None):
    """The loop and stop rule of _fit_coordinate_descent: (W, H, n_iter, violation ratios); trace, a list, receives every
    (W, H) after its iteration."""
    ratios, init, it = [], None, 0
    for it in range(1, max_iter + 1):
        W, H, v = step(X, W, H, update_H, how)
        if trace is not None:
            trace.append((W, H))
        if it == 1:
            init = v
        if init == 0:
            break
        ratios.append(float(v / init))
        if v / init <= tol:
            break
    return W, H, it, ratios


def fit_transform(X, d, seed, tol=TOL, max_iter=MAX_ITER, how="blas", start=None):
    """NMF(d, init=None, solver='cd', tol, max_iter, shuffle=False, random_state=seed).fit(X).transform(X):
    dict(W0, H0, components, n_iter, ratios, Y, transform_n_iter)."""
    W0, H0 = start if start is not None else initialize(X, d, seed, how)
    _W, H, n_iter, ratios = iterate(X, W0, H0, True, tol, max_iter, how)
    Y, _H, t_iter, _r = iterate(X, np.zeros((X.shape[0], d)), H, False, tol, max_iter, how)
    return {"W0": W0, "H0": H0, "components": H, "n_iter": n_iter, "ratios": ratios, "Y": Y, "transform_n_iter": t_iter}
