"""Plain numpy restatement of exact t-SNE as the reference's PY-TSNE runs it (frisk/tsne.py), for the t-SNE tests:
affinities (direct-difference distances, the per-row bisection on beta, symmetrise, normalise, clamp) and one optimiser step,
with a per-entry forward-error bound on the gradient and on the state after the step.

The reference forms squared distances as |a|^2 + |b|^2 - 2 a.b; this restatement and the GPU kernels take direct differences.
step() reports a bound that covers both the rounding of any fixed summation order (c n eps times the sums of absolute terms)
and the difference between the two forms (gram=True), so the same bound compares the GPU with the reference's own states.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
Q_MIN = 1e-12
Q_FLOOR = Q_MIN * 0.25          # fl(1e-12) / 4: the reference's P after iteration 100 is max(p, 1e-12 / 4), bit for bit
H_TOL, MAX_TRIES = 1e-5, 50
STOP_EXAGGERATION, MOMENTUM_SWITCH, ETA, MIN_GAIN = 100, 20, 500.0, 0.01


def sqdist(A):
    """D_ij = sum_k (a_ik - a_jk)^2, the terms added in k order."""
    D = np.zeros((A.shape[0], A.shape[0]))
    for k in range(A.shape[1]):
        t = A[:, k][:, None] - A[:, k][None, :]
        D += t * t
    return D


def affinities(X, perplexity):
    """(beta, tries, q) of x2p + symmetrise + normalise, q = max(p, 1e-12 / 4); every row's bisection as the reference's."""
    n = X.shape[0]
    D = sqdist(X)
    off = ~np.eye(n, dtype=bool)
    logU = np.log(perplexity)

    def hbeta(b):
        P = np.where(off, np.exp(-D * b[:, None]), 0.0)
        sumP = P.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            H = np.log(sumP) + b * (D * P).sum(axis=1) / sumP
        return H, P, sumP

    beta = np.ones(n)
    bmin, bmax = np.full(n, -np.inf), np.full(n, np.inf)
    tries = np.zeros(n, dtype=np.int32)
    H, P, sumP = hbeta(beta)
    Hdiff = H - logU
    while True:
        act = (np.abs(Hdiff) > H_TOL) & (tries < MAX_TRIES)
        if not act.any():
            break
        up = act & (Hdiff > 0)
        dn = act & ~(Hdiff > 0)
        b = beta.copy()
        bmin = np.where(up, b, bmin)
        beta = np.where(up, np.where(np.isinf(bmax), b * 2.0, (b + bmax) / 2.0), beta)
        bmax = np.where(dn, b, bmax)
        beta = np.where(dn, np.where(np.isinf(bmin), b / 2.0, (b + bmin) / 2.0), beta)
        Hn, Pn, sn = hbeta(beta)
        H, P, sumP = np.where(act, Hn, H), np.where(act[:, None], Pn, P), np.where(act, sn, sumP)
        Hdiff = H - logU
        tries += act
    P = P / sumP[:, None]
    P = P + P.T
    q = np.maximum(P / P.sum(), Q_FLOOR)
    return beta, tries, q


def q_tolerance(X, beta, c=8.0):
    """Relative bound on q_ij between two implementations that agree on beta: exp(-D beta) moves by beta dD relative, where dD
    covers the rounding of either distance form (the Gram form's cancellation: 4 eps (|x_i|^2 + |x_j|^2)) and of D beta itself,
    for both conditionals p_j|i and p_i|j, plus the row and total sums (n eps).  Never below 1e-12."""
    s = (X * X).sum(axis=1)
    D = sqdist(X)
    a = beta[:, None] * (4.0 * (s[:, None] + s[None, :]) + 2.0 * D)
    return np.maximum(c * EPS * (a + a.T + X.shape[0]), 1e-12)


class Step:
    """One iteration t from (Y, iY, gains): the new state, dY, the cost if (t + 1) % 10 == 0, and bounds."""


def step(Y, iY, gains, q, t, gram=True, q_rel=0.0, c=8.0):
    """One reference iteration t.  Bounds (per entry): dY_bound on |dY - dY_exact|, Y_bound / iY_bound on the new state of any
    implementation whose dY lies within dY_bound and whose gains agree; q_rel is the relative difference allowed between the
    caller's q and the one the compared implementation holds."""
    n, d = Y.shape
    Pm = 4.0 * q if t <= STOP_EXAGGERATION else q
    D = sqdist(Y)
    num = 1.0 / (1.0 + D)
    np.fill_diagonal(num, 0.0)
    S = num.sum()
    Q = np.maximum(num / S, Q_MIN)
    coef = (Pm - Q) * num
    dY = np.empty_like(Y)
    A = np.empty_like(Y)           # sum_j |coef (y_i - y_j)|
    B = np.empty_like(Y)           # sum_j (P + 2Q) num |y_i - y_j|: a few eps on num, Q and S each
    G = np.empty_like(Y)           # the Gram form's change of num: num^2 dD (P + 2Q) |y_i - y_j|
    s = (Y * Y).sum(axis=1)
    dD = 4.0 * EPS * (s[:, None] + s[None, :] + D)
    for k in range(d):
        diff = Y[:, k][:, None] - Y[:, k][None, :]
        dY[:, k] = (coef * diff).sum(axis=1)
        A[:, k] = np.abs(coef * diff).sum(axis=1)
        B[:, k] = ((Pm + 2.0 * Q) * num * np.abs(diff)).sum(axis=1)
        G[:, k] = (num * num * dD * (Pm + 2.0 * Q) * np.abs(diff)).sum(axis=1)
    dY_bound = c * (n * EPS * (A + B) + q_rel * B) + (c * G if gram else 0.0)
    momentum = 0.5 if t < MOMENTUM_SWITCH else 0.8
    flip = (dY > 0) != (iY > 0)
    g = (gains + 0.2) * flip + (gains * 0.8) * ~flip
    g[g < MIN_GAIN] = MIN_GAIN
    niY = momentum * iY - ETA * (g * dY)
    Yn = Y + niY
    Yn = Yn - np.tile(np.mean(Yn, 0), (n, 1))
    iY_bound = ETA * g * dY_bound + c * EPS * (np.abs(niY) + ETA * np.abs(g * dY))
    Y_bound = iY_bound + iY_bound.max(axis=0) + c * EPS * (np.abs(Y) + np.abs(Yn) + np.abs(Yn).max(axis=0))
    out = Step()
    out.Y, out.iY, out.gains, out.dY = Yn, niY, g, dY
    out.dY_bound, out.iY_bound, out.Y_bound = dY_bound, iY_bound, Y_bound
    out.cost = float(np.sum(Pm * np.log(Pm / Q))) if (t + 1) % 10 == 0 else None
    return out


def compare_state(st, Y, iY, gains):
    """(ok entries mask, number of skipped entries): an entry whose gains differ is skipped when |dY| lies within the bound
    (its sign is not decided), and is a failure otherwise."""
    gdiff = gains != st.gains
    undecided = np.abs(st.dY) <= st.dY_bound
    skip = gdiff & undecided
    ok = (np.abs(Y - st.Y) <= st.Y_bound) & (np.abs(iY - st.iY) <= st.iY_bound) & ~gdiff
    return ok | skip, int(skip.sum())
