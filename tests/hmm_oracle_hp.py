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

The second half of the module is the reference of tests/test_hmm_start_cpu.py and tests/test_gpu_hmm_start.py: the deterministic
start (`start`: GaussianHMM2._init in long double, with an account of every 2-means round's assignment and stop-rule margins, which
the conditions on the test inputs are checked on), hmm.py's M step on e_step's posteriors (`m_step`), and whole EM rounds from the
start (`fit_rounds`) - each with its mpmath counterpart (`start_mp`, `fit_rounds_mp`) and the distance between the two.
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
        # (the double the implementations are given, exactly; a model of mpmath numbers - fit_rounds_mp's - is taken as it is)
        f = lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v))      # noqa: E731
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


# ------------------------------------------------------------------------------------- the deterministic start and the M step
def _ld_sum(v):
    """Sum of a long-double array (numpy's pairwise summation: ~1e-19 log2(n) relative)."""
    return np.sum(v, dtype=LD) if v.size else LD(0)


def start(x, min_covar=1e-3):
    """GaussianHMM2._init in long double: exact min and max, 2-means from the extremes (ties to centre 0, an empty cluster keeps its
    centre, numpy.allclose's stop after which the PREVIOUS centres are kept, 100 rounds at most), two-pass variance + min_covar.
    Returns a dict: means (2, ascending), covar, rounds (assignments made), and per round `margin` (smallest | |x - c0| - |x - c1| |
    over the windows that are not exact ties; inf when all are), `ties` (how many are), `gap` (|c1 - c0|) and `stop` (per centre:
    (|shift|, threshold))."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n = x.size
    c = [x.min(), x.max()]
    atol, rtol = LD(1e-8), LD(1e-5)         # (the doubles numpy.allclose is given)
    info = {"rounds": 0, "margin": [], "ties": [], "gap": [], "stop": []}
    for _ in range(100):
        d0, d1 = np.abs(x - c[0]), np.abs(x - c[1])
        lab0 = d0 <= d1
        diff = np.abs(d0 - d1)
        nz = diff[diff != 0]
        info["rounds"] += 1
        info["margin"].append(nz.min() if nz.size else LD(np.inf))
        info["ties"].append(int(n - nz.size))
        info["gap"].append(abs(c[1] - c[0]))
        n0 = int(lab0.sum())
        new = [_ld_sum(x[lab0]) / LD(n0) if n0 else c[0], _ld_sum(x[~lab0]) / LD(n - n0) if n - n0 else c[1]]
        stop = [(abs(new[s] - c[s]), atol + rtol * abs(c[s])) for s in (0, 1)]
        info["stop"].append(stop)
        if all(sh <= th for sh, th in stop):
            break
        c = new
    mu = _ld_sum(x) / LD(n)
    info["means"] = np.array(sorted(c), dtype=LD)
    info["covar"] = _ld_sum((x - mu) ** 2) / LD(n) + LD(min_covar)
    return info


def start_model(st):
    return dict(means=list(st["means"]), covars=[st["covar"], st["covar"]], start=[LD(1) / 2] * 2, trans=[[LD(1) / 2] * 2] * 2)


def m_step(x, post, stats, covars_prior=1e-2):
    """hmm.py's M step in long double on e_step's posteriors and statistics: a model dict of long doubles."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    half = LD(1) / 2
    start = [post[0, j] / (post[0, 0] + post[0, 1]) for j in (0, 1)]
    trans = [[half, half], [half, half]]
    if x.size > 1:
        for i in (0, 1):
            row = stats[4 + 2 * i] + stats[5 + 2 * i]
            if row > 0:
                trans[i] = [stats[4 + 2 * i] / row, stats[5 + 2 * i] / row]
    means = [stats[2 + j] / stats[j] for j in (0, 1)]
    covars = [max((LD(covars_prior) + _ld_sum(post[:, j] * (x - means[j]) ** 2)) / stats[j], LD(1e-300)) for j in (0, 1)]
    return dict(means=means, covars=covars, start=start, trans=trans)


def fit_rounds(x, rounds, min_covar=1e-3, covars_prior=1e-2):
    """`rounds` EM rounds from the start, none stopped early (GaussianHMM2(n_iter=rounds, tol=-1e300).fit): a list of
    (model after round r, log-likelihood of round r's E step) for r = 1 .. rounds, all long double."""
    model = start_model(start(x, min_covar))
    out = []
    for _ in range(rounds):
        post, stats, ll = e_step(x, model)
        model = m_step(x, post, stats, covars_prior)
        out.append((model, ll))
    return out


def start_mp(x, min_covar=1e-3, digits=50):
    """`start` by mpmath at `digits` digits: (means [2], covar, rounds)."""
    import mpmath as mp
    with mp.workdps(digits):
        xs = [mp.mpf(float(v)) for v in np.asarray(x, dtype=np.float64)]
        n = len(xs)
        c = [min(xs), max(xs)]
        atol, rtol = mp.mpf(1e-8), mp.mpf(1e-5)
        rounds = 0
        for _ in range(100):
            rounds += 1
            g = [[], []]
            for v in xs:
                g[0 if abs(v - c[0]) <= abs(v - c[1]) else 1].append(v)
            new = [mp.fsum(g[s]) / len(g[s]) if g[s] else c[s] for s in (0, 1)]
            if all(abs(new[s] - c[s]) <= atol + rtol * abs(c[s]) for s in (0, 1)):
                break
            c = new
        mu = mp.fsum(xs) / n
        return sorted(c), mp.fsum((v - mu) ** 2 for v in xs) / n + mp.mpf(float(min_covar)), rounds


def fit_rounds_mp(x, rounds, min_covar=1e-3, covars_prior=1e-2, digits=50):
    """`fit_rounds` by mpmath (the unscaled e_step_mp): a list of (model of mpmath numbers, log-likelihood)."""
    import mpmath as mp
    with mp.workdps(digits):
        means, covar, _r = start_mp(x, min_covar, digits)
        half = mp.mpf(1) / 2
        model = dict(means=means, covars=[covar, covar], start=[half, half], trans=[[half, half], [half, half]])
        xs = [mp.mpf(float(v)) for v in np.asarray(x, dtype=np.float64)]
        out = []
        for _ in range(rounds):
            post, stats, ll = e_step_mp(x, model, digits)
            start_p = [post[0][j] / (post[0][0] + post[0][1]) for j in (0, 1)]
            trans = [[half, half], [half, half]]
            if len(xs) > 1:
                for i in (0, 1):
                    row = stats[4 + 2 * i] + stats[5 + 2 * i]
                    if row > 0:
                        trans[i] = [stats[4 + 2 * i] / row, stats[5 + 2 * i] / row]
            mu = [stats[2 + j] / stats[j] for j in (0, 1)]
            cv = [max((mp.mpf(float(covars_prior)) + mp.fsum(g[j] * (v - mu[j]) ** 2 for g, v in zip(post, xs))) / stats[j], mp.mpf(1e-300))
                  for j in (0, 1)]
            model = dict(means=mu, covars=cv, start=start_p, trans=trans)
            out.append((model, ll))
        return out


def to_mp(v):
    import mpmath as mp
    return v if isinstance(v, mp.mpf) else mp.mpf(repr_ld(v))


def start_distance_from_mp(x, min_covar=1e-3):
    """(means, covar), each relative to max(1, |value|): how far `start` lies from start_mp (whose round count it must share)."""
    import mpmath as mp
    st = start(x, min_covar)
    mm, mc, mr = start_mp(x, min_covar)
    assert mr == st["rounds"], (mr, st["rounds"])
    with mp.workdps(50):
        dm = max(abs(to_mp(st["means"][j]) - mm[j]) / max(1, abs(mm[j])) for j in (0, 1))
        return float(dm), float(abs(to_mp(st["covar"]) - mc) / max(1, abs(mc)))


def rounds_distance_from_mp(x, rounds, min_covar=1e-3, covars_prior=1e-2):
    """{r: (parameters, log-likelihood)} for r in `rounds`: how far fit_rounds lies from fit_rounds_mp, a field's largest difference
    relative to max(1, its largest |entry|), the log-likelihood's to max(1, |ll|)."""
    import mpmath as mp
    mine, theirs = fit_rounds(x, max(rounds), min_covar, covars_prior), fit_rounds_mp(x, max(rounds), min_covar, covars_prior)
    flat = lambda m: {"means": m["means"], "covars": m["covars"], "start": m["start"], "trans": [v for row in m["trans"] for v in row]}      # noqa: E731
    out = {}
    with mp.workdps(50):
        for r in rounds:
            (a, lla), (b, llb) = mine[r - 1], theirs[r - 1]
            a, b = flat(a), flat(b)
            dp = max(abs(to_mp(u) - v) / max(1, max(abs(w) for w in b[f])) for f in b for u, v in zip(a[f], b[f]))
            out[r] = (float(dp), float(abs(to_mp(lla) - llb) / max(1, abs(llb))))
    return out
