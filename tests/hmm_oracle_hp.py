"""Extended-precision E step of the 2-state Gaussian HMM  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The reference of tests/test_hmm_estep_cpu.py and tests/test_gpu_hmm_estep.py: a SERIAL forward-backward in x87 extended precision
(np.longdouble, 64-bit mantissa), one Python step per window and no pieces:
  * emissions in long double, relative to the larger of the two per window (so one of them is exactly 1);
  * forward and backward vectors renormalised at every step;
  * the log-likelihood as a long-double sum of the logarithms of the scales (and of the emissions' own scales);
  * posteriors and transition posteriors normalised per window.
It shares no code and no layout with frisk_amd/csrc/hmm_host.h or hmm_kernels.h.

Not log-space: a log-space recursion carries scores that grow like 3 n, so its ABSOLUTE error grows with n and shows in the
transition sums from n ~ 1000 on.  `e_step_logspace` is kept as a second opinion for n <= 200 only; `e_step_mp` (mpmath, 50 digits,
unscaled) is what qualifies this module (tests/test_hmm_estep_cpu.py): its distance from mpmath must be at least 16 times smaller
than the tolerance it is used to enforce.
"""
import numpy as np

assert np.finfo(np.longdouble).nmant >= 63, (
    "the HMM reference needs an extended-precision long double (x87, 64-bit mantissa); this platform's has %d bits: "
    "the E-step tests would silently compare double against double" % (np.finfo(np.longdouble).nmant + 1))

LD = np.longdouble
LOG2PI = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))


def _model(model):
    mu = [LD(v) for v in model["means"]]
    cv = [LD(v) for v in model["covars"]]
    pi = [LD(v) for v in model["start"]]
    A = [[LD(v) for v in row] for row in model["trans"]]
    return mu, cv, pi, A


def emissions(x, model):
    """(b (n x 2, the larger entry of a row exactly 1), mx (n)): density_j(x_t) = exp(mx_t) b_tj."""
    mu, cv, _pi, _A = _model(model)
    x = np.asarray(x, dtype=np.float64).astype(LD)
    l0 = -(LOG2PI + np.log(cv[0]) + (x - mu[0]) ** 2 / cv[0]) / LD(2)
    l1 = -(LOG2PI + np.log(cv[1]) + (x - mu[1]) ** 2 / cv[1]) / LD(2)
    mx = np.maximum(l0, l1)
    return np.stack((np.exp(l0 - mx), np.exp(l1 - mx)), axis=1), mx


def e_step(x, model):
    """(posteriors n x 2, stats[8] = sums of gamma_0, gamma_1, gamma_0 x, gamma_1 x, xi_00, xi_01, xi_10, xi_11, loglik), all long double."""
    _mu, _cv, pi, A = _model(model)
    a00, a01, a10, a11 = A[0][0], A[0][1], A[1][0], A[1][1]
    b, mx = emissions(x, model)
    n = b.shape[0]
    b0, b1 = list(b[:, 0]), list(b[:, 1])
    al0, al1, logs = [None] * n, [None] * n, [None] * n
    v0, v1 = pi[0] * b0[0], pi[1] * b1[0]
    s = v0 + v1
    v0, v1 = v0 / s, v1 / s
    al0[0], al1[0], logs[0] = v0, v1, s
    for t in range(1, n):
        w0, w1 = (v0 * a00 + v1 * a10) * b0[t], (v0 * a01 + v1 * a11) * b1[t]
        s = w0 + w1
        v0, v1 = w0 / s, w1 / s
        al0[t], al1[t], logs[t] = v0, v1, s
    ll = np.sum(np.log(np.array(logs, dtype=LD))) + np.sum(mx)
    be0, be1 = [None] * n, [None] * n
    v0 = v1 = LD(1) / LD(2)
    be0[n - 1], be1[n - 1] = v0, v1
    for t in range(n - 1, 0, -1):
        c0, c1 = b0[t] * v0, b1[t] * v1
        w0, w1 = a00 * c0 + a01 * c1, a10 * c0 + a11 * c1
        s = w0 + w1
        v0, v1 = w0 / s, w1 / s
        be0[t - 1], be1[t - 1] = v0, v1
    al = np.stack((np.array(al0, dtype=LD), np.array(al1, dtype=LD)), axis=1)
    be = np.stack((np.array(be0, dtype=LD), np.array(be1, dtype=LD)), axis=1)
    post = al * be
    post /= post.sum(axis=1, keepdims=True)
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    stats = np.zeros(8, dtype=LD)
    stats[0:2] = post.sum(axis=0)
    stats[2:4] = (post * xl[:, None]).sum(axis=0)
    if n > 1:
        Am = np.array(A, dtype=LD)
        xi = al[:-1, :, None] * Am[None] * (b[1:] * be[1:])[:, None, :]
        xi /= xi.sum(axis=(1, 2), keepdims=True)
        stats[4:8] = xi.sum(axis=0).ravel()
    return post, stats, ll


def e_step_logspace(x, model):
    """The same quantities by a log-space long-double recursion: a second opinion for n <= 200 (see the module text)."""
    mu, cv, pi, A = _model(model)
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n = x.size
    assert n <= 200
    with np.errstate(divide="ignore"):
        lt, ls = np.log(np.array(A, dtype=LD)), np.log(np.array(pi, dtype=LD))
    lb = np.stack([-(LOG2PI + np.log(cv[j]) + (x - mu[j]) ** 2 / cv[j]) / LD(2) for j in (0, 1)], axis=1)

    def lse(a, axis):
        m = np.max(a, axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, LD(0))
        with np.errstate(divide="ignore"):
            return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))
    fwd = np.empty((n, 2), dtype=LD)
    fwd[0] = ls + lb[0]
    for t in range(1, n):
        fwd[t] = lse(fwd[t - 1][:, None] + lt, 0) + lb[t]
    bwd = np.zeros((n, 2), dtype=LD)
    for t in range(n - 2, -1, -1):
        bwd[t] = lse(lt + (lb[t + 1] + bwd[t + 1])[None, :], 1)
    ll = lse(fwd[-1], 0)
    post = np.exp(fwd + bwd - ll)
    post /= post.sum(axis=1, keepdims=True)
    stats = np.zeros(8, dtype=LD)
    stats[0:2] = post.sum(axis=0)
    stats[2:4] = (post * x[:, None]).sum(axis=0)
    if n > 1:
        xi = np.exp(fwd[:-1, :, None] + lt[None] + (lb[1:] + bwd[1:])[:, None, :] - ll)
        xi /= xi.sum(axis=(1, 2), keepdims=True)
        stats[4:8] = xi.sum(axis=0).ravel()
    return post, stats, ll


def e_step_mp(x, model, digits=50):
    """The same quantities by mpmath at `digits` digits, unscaled (mpmath's exponent range has no practical end): what qualifies
    e_step.  Returns mpmath numbers: (list of [g0, g1], list of 8, ll)."""
    import mpmath as mp
    with mp.workdps(digits):
        f = lambda v: mp.mpf(float(v))      # noqa: E731  (the double the implementations are given, exactly)
        mu, cv, pi = [f(v) for v in model["means"]], [f(v) for v in model["covars"]], [f(v) for v in model["start"]]
        A = [[f(v) for v in row] for row in model["trans"]]
        xs = [f(v) for v in np.asarray(x, dtype=np.float64)]
        n = len(xs)
        b = [[mp.exp(-(mp.log(2 * mp.pi) + mp.log(cv[j]) + (xt - mu[j]) ** 2 / cv[j]) / 2) for j in (0, 1)] for xt in xs]
        al = [[pi[0] * b[0][0], pi[1] * b[0][1]]]
        for t in range(1, n):
            p = al[-1]
            al.append([(p[0] * A[0][0] + p[1] * A[1][0]) * b[t][0], (p[0] * A[0][1] + p[1] * A[1][1]) * b[t][1]])
        be = [None] * n
        be[n - 1] = [mp.mpf(1), mp.mpf(1)]
        for t in range(n - 1, 0, -1):
            c0, c1 = b[t][0] * be[t][0], b[t][1] * be[t][1]
            be[t - 1] = [A[0][0] * c0 + A[0][1] * c1, A[1][0] * c0 + A[1][1] * c1]
        L = al[-1][0] + al[-1][1]
        post = [[al[t][0] * be[t][0] / L, al[t][1] * be[t][1] / L] for t in range(n)]
        stats = [mp.fsum(g[0] for g in post), mp.fsum(g[1] for g in post),
                 mp.fsum(g[0] * xt for g, xt in zip(post, xs)), mp.fsum(g[1] * xt for g, xt in zip(post, xs))]
        for i in (0, 1):
            for j in (0, 1):
                stats.append(mp.fsum(al[t - 1][i] * A[i][j] * b[t][j] * be[t][j] / L for t in range(1, n)))
        return post, stats, mp.log(L)


def distance_from_mp(x, model):
    """(posterior abs, statistics rel to max(1, |value|), loglik rel to max(1, |ll|)): how far e_step lies from e_step_mp."""
    import mpmath as mp
    post, stats, ll = e_step(x, model)
    mpost, mstats, mll = e_step_mp(x, model)
    with mp.workdps(50):
        g = lambda v: mp.mpf(repr_ld(v))      # noqa: E731
        dp = max(abs(g(post[t, j]) - mpost[t][j]) for t in range(len(mpost)) for j in (0, 1))
        ds = max(abs(g(stats[k]) - mstats[k]) / max(1, abs(mstats[k])) for k in range(8))
        dl = abs(g(ll) - mll) / max(1, abs(mll))
        return float(dp), float(ds), float(dl)


def repr_ld(v):
    """A long double as a decimal string that mpmath reads back exactly enough (25 significant digits > 64 bits)."""
    return np.format_float_scientific(LD(v), precision=24, unique=False)
