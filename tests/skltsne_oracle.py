"""Oracles of the SKL-TSNE tests, numpy only (no sklearn, no GPU): the seeded inputs of tests/golden/skltsne/skltsne.npz, a transcription of
sklearn 1.7's _gradient_descent loop that exposes its state (tools/make_skltsne_golden.py records sklearn's objectives through it,
and tests/test_skltsne_cpu.py holds it bit for bit to sklearn's own loop), and extended-precision (long double) restatements of
the affinities and of both objectives with direct-difference distances, against which the tool calibrates the test bounds.
"""
import numpy as np

LD = np.longdouble
EPS64 = np.finfo(np.float64).eps
EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
LEARNING_RATE, MIN_GAIN = 1000.0, 0.01


def make_X(seed, n, f, kind="dirichlet"):
    """The inputs of a golden case: seeded Dirichlet proportion rows (n x f, float64), like the other projection goldens.
    'duplicates': rows 1, 2 and 3 are copies of row 0's neighbour row 1 (three identical rows); 'simplex': the unit vectors (every
    pair of rows at squared distance 2); 'uniform': uniform on [0, 1) (for f = 1, where a Dirichlet row is the constant 1)."""
    if kind == "simplex":
        return np.eye(n, f)
    if kind == "uniform":
        return np.random.RandomState(seed).uniform(size=(n, f))
    X = np.random.RandomState(seed).dirichlet(np.full(f, 0.7), size=n)
    if kind == "duplicates":
        X[2] = X[1]
        X[3] = X[1]
    return np.ascontiguousarray(X)


def n_neighbors(n, perplexity):
    return min(n - 1, int(3.0 * perplexity + 1))


def random_start(seed, n, d):
    """sklearn's init='random' from RandomState(seed), float32."""
    return np.ascontiguousarray(1e-4 * np.random.RandomState(seed).standard_normal(size=(n, d)).astype(np.float32), dtype=np.float32)


def synthetic_state(seed, n, d, which):
    """(Y, update, gains), float32 n x d, of the single-step cases too large to store a recorded state for: 'start' is the start of a
    run, 'mid' a state as stage 2 sees it (an embedding of scale 3, updates of scale 0.01, gains from the clamp to above 2)."""
    if which == "start":
        return random_start(seed, n, d), np.zeros((n, d), np.float32), np.ones((n, d), np.float32)
    rs = np.random.RandomState(seed)
    Y = (3.0 * rs.standard_normal(size=(n, d))).astype(np.float32)
    U = (1e-2 * rs.standard_normal(size=(n, d))).astype(np.float32)
    G = rs.choice(np.array([0.01, 0.8, 1.0, 1.2, 2.5], dtype=np.float32), size=(n, d)).astype(np.float32)
    return Y, U, G


# ------------------------------------------------------------------------------------------------ _gradient_descent, transcribed
def gd_step(p, update, gains, grad, momentum):
    """One pass of the loop body of _gradient_descent after the objective, on float32 arrays, in place on copies: returns (p,
    update, gains, grad * gains)."""
    p, update, gains, grad = p.copy(), update.copy(), gains.copy(), grad.copy()
    inc = update * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, MIN_GAIN, np.inf, out=gains)
    grad *= gains
    update = momentum * update - LEARNING_RATE * grad
    p += update
    return p, update, gains, grad


def gradient_descent(objective, p0, it, max_iter, n_iter_check, n_iter_without_progress, momentum, min_grad_norm=1e-7, args=(),
                     kwargs=None, record=None):
    """sklearn's _gradient_descent (learning_rate 1000, min_gain 0.01) with a hook: record(i, p, update, gains), if given, is
    called before iteration i with the state it starts from.  Returns (p, error, i, update, gains, checks) with checks the list
    of (i, error, grad_norm) of every convergence check."""
    from scipy import linalg
    kwargs = dict(kwargs or {})
    p = p0.copy().ravel()
    update = np.zeros_like(p)
    gains = np.ones_like(p)
    error = np.finfo(float).max
    best_error = np.finfo(float).max
    best_iter = i = it
    checks = []
    for i in range(it, max_iter):
        if record is not None:
            record(i, p, update, gains)
        check_convergence = (i + 1) % n_iter_check == 0
        kwargs["compute_error"] = check_convergence or i == max_iter - 1
        error, grad = objective(p, *args, **kwargs)
        p, update, gains, grad = gd_step(p, update, gains, grad, momentum)
        if check_convergence:
            grad_norm = linalg.norm(grad)
            checks.append((i, float(error), float(grad_norm)))
            if error < best_error:
                best_error = error
                best_iter = i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return p, error, i, update, gains, checks


def tsne_descent(objective, Y0, P, dof, exaggerate, unexaggerate, extra_kwargs=None, record=None, max_iter=1000):
    """TSNE._tsne's two stages through gradient_descent.  exaggerate(P) / unexaggerate(P) are sklearn's in-place P *= 4 and P /= 4.
    record(stage, i, p, update, gains).  Returns (Y, kl_divergence, n_iter, checks of stage 1, checks of stage 2)."""
    n, d = Y0.shape
    kw = dict(extra_kwargs or {})
    kw["skip_num_points"] = 0
    rec1 = None if record is None else (lambda i, p, u, g: record(1, i, p, u, g))
    rec2 = None if record is None else (lambda i, p, u, g: record(2, i, p, u, g))
    P = exaggerate(P)
    p, kl, it, _u, _g, c1 = gradient_descent(objective, Y0.ravel(), 0, 250, 50, 250, 0.5, args=[P, dof, n, d], kwargs=kw, record=rec1)
    P = unexaggerate(P)
    c2 = []
    if it < 250 or max_iter - 250 > 0:
        p, kl, it, _u, _g, c2 = gradient_descent(objective, p, it + 1, max_iter, 50, 30, 0.8, args=[P, dof, n, d], kwargs=kw,
                                                 record=rec2)
    return p.reshape(n, d), kl, it, c1, c2


# ------------------------------------------------------------------------------------------------ long double restatements
def sqdist_direct(X):
    """Squared Euclidean distances by direct differences in float64 (k in order), as the device sums them."""
    n, f = X.shape
    D = np.zeros((n, n))
    for k in range(f):
        t = X[:, k][:, None] - X[:, k][None, :]
        D += t * t
    return D


def ld_bisect(D32, perplexity, dense):
    """_binary_search_perplexity in long double on float32 squared distances D32 (n x m).  dense: m = n and j == i is left out.
    Returns (P long double n x m, beta of the final probabilities, step that met the tolerance or 100)."""
    n, m = D32.shape
    D = D32.astype(LD)
    logU = np.log(LD(np.float32(perplexity)))
    tol = LD(np.float32(1e-5))
    mask = np.ones((n, m), dtype=bool)
    if dense:
        mask[np.arange(n), np.arange(n)] = False
    beta = np.ones(n, dtype=LD)
    bmin = np.full(n, -np.inf, dtype=LD)
    bmax = np.full(n, np.inf, dtype=LD)
    P = np.zeros((n, m), dtype=LD)
    beta_used = beta.copy()
    steps = np.full(n, 100, dtype=np.int32)
    live = np.ones(n, dtype=bool)
    for step in range(100):
        r = np.nonzero(live)[0]
        if r.size == 0:
            break
        # each exponential passes through float64, so that it underflows (and goes subnormal) where sklearn's does: a row whose
        # exponentials all underflow takes the sum == 0 branch, which long double's range would never reach
        e = np.where(mask[r], np.exp(-D[r] * beta[r, None]).astype(np.float64).astype(LD), LD(0))
        s = e.sum(axis=1)
        s = np.where(s == 0, LD(np.float32(1e-8)), s)
        Pr = e / s[:, None]
        H = np.log(s) + beta[r] * (D[r] * Pr).sum(axis=1)
        diff = H - logU
        P[r] = Pr
        beta_used[r] = beta[r]
        done = np.abs(diff) <= tol
        steps[r[done]] = step
        live[r[done]] = False
        up = (diff > 0) & ~done
        dn = ~(diff > 0) & ~done
        ru, rd = r[up], r[dn]
        bmin[ru] = beta[ru]
        beta[ru] = np.where(np.isinf(bmax[ru]), beta[ru] * 2, (beta[ru] + bmax[ru]) / 2)
        bmax[rd] = beta[rd]
        beta[rd] = np.where(np.isinf(bmin[rd]), beta[rd] / 2, (beta[rd] + bmin[rd]) / 2)
    return P, beta_used, steps


def ld_joint_dense(C):
    """_joint_probabilities' last three lines on the conditional C (long double), as an n x n matrix with a zero diagonal."""
    P = C + C.T
    s = np.maximum(P.sum(), LD(EPS64))
    P = np.maximum(P / s, LD(EPS64))
    P[np.arange(len(P)), np.arange(len(P))] = 0
    return P


def _pairs(Y32, dof, bh):
    Y = Y32.astype(LD)
    diff = Y[:, None, :] - Y[None, :, :]
    s = (diff * diff).sum(axis=2)
    fd = LD(dof)
    if bh:
        q = (fd / (fd + s)) ** ((fd + 1) / 2)
    else:
        q = (s / fd + 1) ** ((fd + 1) / -2)
    q[np.arange(len(Y)), np.arange(len(Y))] = 0
    diff32 = (Y32[:, None, :] - Y32[None, :, :]).astype(LD)        # sklearn multiplies the weights with float32 differences
    return q, diff32


def error_scale(terms, p):
    """The natural magnitude of the rounding error of sum p log(p / Q): a term's own size, plus p, because the ratio p / Q carries
    a relative rounding error that the logarithm passes on as an ABSOLUTE one (d log r = dr / r), so a term errs by p x a few eps
    however small log(p / Q) is - near the optimum, where p / Q is close to 1, that part is all there is."""
    return np.abs(terms).sum() + np.abs(p).sum()


def ld_objective_exact(Y32, P, dof):
    """_kl_divergence in long double.  P: n x n float64 (already exaggerated, zero diagonal).  Returns (error, gradient n x d, the
    scale of the error's rounding: see error_scale)."""
    num, diff32 = _pairs(Y32, dof, False)
    Pl = P.astype(LD)
    Q = np.maximum(num / num.sum(), LD(EPS64))
    off = ~np.eye(len(P), dtype=bool)
    terms = np.where(off, Pl * np.log(np.maximum(Pl, LD(EPS64)) / Q), LD(0))
    c = LD(2) * (dof + 1) / dof
    grad = c * np.einsum("ij,ijk->ik", np.where(off, (Pl - Q) * num, LD(0)), diff32)
    return terms.sum(), grad, error_scale(terms, Pl[off])


def ld_objective_bh(Y32, indptr, indices, val32, dof):
    """_kl_divergence_bh with every pair visited (angle -> 0), in long double.  val32: the float32 CSR values (already exaggerated).
    Returns (error, gradient n x d, the scale of the error's rounding: see error_scale)."""
    n = len(Y32)
    q, diff32 = _pairs(Y32, dof, True)
    sumQ = np.maximum(q.sum(), LD(EPS64))
    neg = np.einsum("ij,ijk->ik", q * q, diff32)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    p = val32.astype(LD)
    qn = q[rows, indices]
    terms = p * np.log(np.maximum(p, LD(TINY32)) / np.maximum(qn / sumQ, LD(TINY32)))
    pos = np.zeros_like(neg)
    np.add.at(pos, rows, (p * qn)[:, None] * diff32[rows, indices])
    c = LD(2) * (dof + 1) / dof
    return terms.sum(), c * (pos - neg / sumQ), error_scale(terms, p)
