"""Cases, reference access and the comparison routine of the E-step tests (shared by tools/make_golden_hmm_estep.py,
tests/test_hmm_estep_cpu.py and tests/test_gpu_hmm_estep.py).  Test infrastructure only.

Models are FIXED (never fitted; also written to tests/golden/hmm_estep.json as data).  Inputs are regenerated from their seeds and
their sha256 recorded.  Two input families:
  * "regimes": two-regime draws of the model's own means and variances (hmm_gpu_cases._two_regimes), clipped at 1e-4, with one
    window at 2.5 in the middle;
  * "cuts": the same draws (another seed) with outliers ON the device layout's cuts: at several cuts c = a_(p+1) the windows
    c - 2, c - 1, c, c + 1 are far above / far below both means in turn, so that a scaled emission underflows to exactly 0 at the
    last window of piece p and at the first of piece p + 1 (with the `apart` model consecutive emissions are (0, 1), (1, 0),
    (0, 1), (1, 0) across the cut, and its 1e-70 transitions drive the forward walk's held product below 1e-200); the first and
    last window of the sequence carry one too.
Sizes up to 2049 are compared window by window with the oracle at test time; from 4095 on the oracle ran once
(tools/make_golden_hmm_estep.py) and its nine statistics and the posteriors of a fixed sample of windows are recorded.
"""
import functools
import json
import os

import numpy as np

import hmm_gpu_cases as H
import hmm_piece_model as PM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLD, "hmm_estep.json")
NPZ = os.path.join(GOLD, "hmm_estep", "large.npz")

FACTOR = H.FACTOR         # 8: the project's margin for this model (tests/hmm_gpu_cases.py)
ORACLE_MARGIN = 16        # the oracle's own distance from mpmath must be this many times below the tolerance
FLIP = 0.1                # regime flips per window of the draws: runs of ~10 windows, so that no run outlasts double's range under `forbidden`
HI, LO = 2.5, -1.5        # the outliers: far above and far below both means of every model

MODELS = {
    "kld": H.KLD_MODEL,
    "sticky": dict(means=[0.04, 0.13], covars=[2e-4, 1.5e-3], start=[1 - 1e-12, 1e-12], trans=[[1.0, 1e-30], [1e-25, 1.0]]),
    "tinyvar": dict(means=[0.04, 0.13], covars=[1e-8, 1e-3], start=[0.5, 0.5], trans=[[0.9, 0.1], [0.2, 0.8]]),
    # state 1 absorbing (1 -> 0 impossible).  The mirror image (0 -> 1 impossible) is no usable case: an outlier, which only state 1
    # can emit, then forces state 1 on every window BEFORE it, and the forward vector's state-1 entry underflows double (and long
    # double) over the first long stretch of low windows - the sequence is impossible to the arithmetic, not to the kernel
    "forbidden": dict(means=[0.04, 0.13], covars=[2e-4, 1.5e-3], start=[0.5, 0.5], trans=[[0.9, 0.1], [0.0, 1.0]]),
    "equal": dict(means=[0.1, 0.1], covars=[1e-3, 1e-3], start=[0.5, 0.5], trans=[[0.5, 0.5], [0.5, 0.5]]),
    # equal variances and means 1 apart: an outlier ABOVE leaves state 1 alone, one BELOW state 0 alone ((0, 1) and (1, 0), exactly)
    "apart": dict(means=[0.5, 1.5], covars=[1e-3, 1e-3], start=[0.5, 0.5], trans=[[1.0, 1e-70], [1e-75, 1.0]]),
}
FAMILIES = ("regimes", "cuts")
SMALL = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 2049)      # .. 64: the first size with two device pieces
LARGE = (4095, 4096, 4097,                                                      # the host form's first cut (n / 2048)
         524287, 524288, 524289, 524288 + 16383)                                # the cap P == PIECES; pieces of 32 and 33 interleaved
QUANTITIES = ("posterior", "statistics", "loglik")


def case_id(model, family, n):
    return "%s-%s-%d" % (model, family, n)


def all_cases(sizes):
    return [(m, f, n) for m in MODELS for f in FAMILIES for n in sizes]


def _seed(model, family, n):
    return [list(MODELS).index(model), FAMILIES.index(family), n, 20260]


def case_input(model, family, n):
    rng = np.random.default_rng(_seed(model, family, n))
    x = H._two_regimes(rng, n, FLIP, MODELS[model]).clip(1e-4, None)
    if family == "regimes":
        x[n // 2] = HI
    else:
        P = PM.pieces_of(n)
        cut = PM.bounds(n, P)
        for p in sorted({0, 1, 2, P // 2, P - 3, P - 2} & set(range(P - 1))):
            c = cut[p + 1]
            x[c - 2], x[c - 1], x[c], x[c + 1] = HI, LO, HI, LO
        x[0] = LO
        if n > 1:
            x[n - 1] = HI
    return np.ascontiguousarray(x, dtype=np.float64)


def sample_windows(n):
    """The windows of a large case whose posteriors are recorded: four on each side of the first eight and the last eight cuts
    of the device layout, and 512 seeded positions."""
    P = PM.pieces_of(n)
    cut = PM.bounds(n, P)
    inner = list(range(1, P))
    near = [c + d for p in sorted(set(inner[:8] + inner[-8:])) for c in (cut[p],) for d in range(-4, 4)]
    rnd = np.random.default_rng([n, 512]).integers(0, n, 512).tolist()
    return np.array(sorted(set(t for t in near + rnd if 0 <= t < n)), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(JSON))


@functools.lru_cache(maxsize=None)
def _large():
    return np.load(NPZ)


@functools.lru_cache(maxsize=None)
def reference(model, family, n):
    """(windows or None for all, posteriors of those windows, stats[8], loglik) as float64 roundings of the oracle's long doubles
    (their rounding, 1.1e-16 relative, is counted in the oracle's recorded error)."""
    if n in LARGE:
        z, k = _large(), case_id(model, family, n)
        return sample_windows(n), z[k + "/post"], z[k + "/stats"][:8], float(z[k + "/stats"][8])
    import hmm_oracle_hp as O
    post, stats, ll = O.e_step(case_input(model, family, n), MODELS[model])
    return None, post.astype(np.float64), stats.astype(np.float64), float(ll)


def errors(n, got, ref):
    """got = (post n x 2, stats[8], ll).  {quantity: error}, and the worst window: posteriors absolute, statistics relative to
    max(1, |value|), log-likelihood relative to max(1, |ll|).  Anything non-finite is an infinite error."""
    post, stats, ll = got
    win, rpost, rstats, rll = ref
    mine = np.asarray(post, dtype=np.float64) if win is None else np.asarray(post, dtype=np.float64)[win]
    d = np.abs(mine - rpost)
    d = np.where(np.isfinite(d), d, np.inf)
    w = int(np.argmax(d.max(axis=1)))
    ds = np.abs(np.asarray(stats, dtype=np.float64) - rstats) / np.maximum(1.0, np.abs(rstats))
    dl = abs(ll - rll) / max(1.0, abs(rll))
    e = {"posterior": float(d.max()), "statistics": float(np.where(np.isfinite(ds), ds, np.inf).max()),
         "loglik": float(dl) if np.isfinite(dl) else float("inf")}
    return e, (w if win is None else int(win[w]))


def where(n, t, pieces=PM.pieces_of):
    """(piece, offset inside the piece) of window t in the layout `pieces`."""
    P = pieces(n)
    cut = PM.bounds(n, P)
    p = int(np.searchsorted(cut, t, side="right")) - 1
    return p, t - cut[p]


def check(model, family, n, got, tol=None, what="device"):
    """Assert got within the tolerance of the reference; the message names the case, the worst window, its piece and offset."""
    tol = tol or golden()["tolerance"]
    e, t = errors(n, got, reference(model, family, n))
    p, off = where(n, t)
    msg = "%s %s: posterior %.3g (allowed %.3g; worst window %d = piece %d of %d, offset %d), statistics %.3g (%.3g), loglik %.3g (%.3g)" % (
        what, case_id(model, family, n), e["posterior"], tol["posterior"], t, p, PM.pieces_of(n), off, e["statistics"],
        tol["statistics"], e["loglik"], tol["loglik"])
    assert all(e[q] <= tol[q] for q in QUANTITIES), msg
    return e, msg


def structure(n, got, tol=None):
    """Posteriors in [0, 1] with rows summing to 1 within 4 ulp; sum gamma = n and sum xi = n - 1 within the statistics tolerance."""
    tol = tol or golden()["tolerance"]
    post, stats, _ll = got
    assert post.shape == (n, 2) and np.all(post >= 0.0) and np.all(post <= 1.0)
    assert np.max(np.abs(post.sum(axis=1) - 1.0)) <= 4 * np.finfo(np.float64).eps
    assert abs((stats[0] + stats[1]) - n) <= tol["statistics"] * max(1.0, n)
    assert abs(stats[4:8].sum() - (n - 1)) <= tol["statistics"] * max(1.0, n - 1)


def host_e_step(model, x, native=True):
    return H.model_of(MODELS[model], native).e_step(x)
