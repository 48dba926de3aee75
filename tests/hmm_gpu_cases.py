"""Seeded inputs of the device-HMM tests, and the CPU-side measurements that qualify them (shared by tools/make_golden_update.py,
tests/test_update_hmm_cpu.py and tests/test_gpu_hmm.py).  Test infrastructure only.

Fit cases: every input is regenerated from its seed (numpy's PCG64 stream; the sha256 of the bytes is recorded in
tests/golden/hmm_gpu.json, so a drifted generator is noticed).  Viterbi cases carry a FIXED model (no fit in the way) and are
kept only while the numpy path decides every step by more than MARGIN - measured here, by the numpy path's own arithmetic.
"""
import hashlib

import numpy as np

from frisk_amd.hmm import GaussianHMM2

PIECES = 16384            # frisk_hmm_gpu::PIECES (csrc/hmm_kernels.h)
VIT_STEPS = 256           # frisk_hmm_gpu::VIT_STEPS
MARGIN = 1e-9             # smallest per-step decision margin of the numpy Viterbi path a test input may have
GAP = 1e-6                # smallest distance of any round's log-likelihood gain from tol a fit input may have
FACTOR = 8                # device tolerance = FACTOR x (numpy specification against host-native spread)

FIT_CASES = {
    # name: (seed, n, flip probability, (mean, sd) low, (mean, sd) high, outlier)
    "clean": (101, 20000, 0.01, (0.03, 0.005), (0.15, 0.010), None),
    "overlap": (102, 20000, 0.02, (0.04, 0.020), (0.08, 0.030), None),
    "outlier": (103, 6000, 0.02, (0.04, 0.010), (0.15, 0.040), 2.5),
    "n1": (104, 1, 0.5, (0.04, 0.010), (0.15, 0.040), None),
    "n2": (105, 2, 0.5, (0.04, 0.010), (0.15, 0.040), None),
    "below_pieces": (106, PIECES - 1, 0.01, (0.03, 0.010), (0.12, 0.050), None),
    "at_pieces": (107, PIECES, 0.01, (0.03, 0.010), (0.12, 0.050), None),
    "above_pieces": (108, PIECES + 1, 0.01, (0.03, 0.010), (0.12, 0.050), None),
    # (below_pieces / at_pieces / above_pieces bracket n = PIECES, where P is 511 or 512 - NOT the cap P == PIECES, which is reached at
    # n = 32 * PIECES = 524288 and is bracketed by tests/hmm_estep_cases.py's sizes)
    "rows_3m": (109, 3000000, 0.002, (0.03, 0.010), (0.12, 0.050), None),
}
BIG = ("rows_3m",)        # the numpy specification takes minutes on these: its fit is recorded, not recomputed by the tests


def fit_input(name):
    seed, n, flip, lo, hi, outlier = FIT_CASES[name]
    rng = np.random.default_rng(seed)
    st = np.cumsum(rng.random(n) < flip) % 2
    x = np.where(st == 0, rng.normal(lo[0], lo[1], n), rng.normal(hi[0], hi[1], n)).clip(1e-4, None)
    if outlier is not None:
        x[n // 2] = outlier                 # one window far from both means
    return np.ascontiguousarray(x, dtype=np.float64)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class RecordingHMM(GaussianHMM2):
    """The numpy specification, remembering the log-likelihood of every round's E step."""

    def __init__(self, **kw):
        super().__init__(native=False, **kw)
        self.lls = []

    def _forward_backward(self, b):
        out = super()._forward_backward(b)
        self.lls.append(float(out[2]))
        return out


def native_lls(x, rounds, **kw):
    """Log-likelihoods of rounds 1..rounds of the host-native fit (round r's is that of the model after r - 1 M steps)."""
    return [GaussianHMM2(n_iter=r, tol=-1e300, native=True, **kw).fit(x).loglik_ for r in range(1, rounds + 1)]


def gap_from_tol(lls, tol=1e-2):
    """Smallest |gain - tol| over the rounds that test a finite gain (inf when there is none)."""
    gains = np.diff(np.asarray(lls, dtype=float))
    return float(np.min(np.abs(gains - tol))) if gains.size else float("inf")


FIELDS = ("means_", "covars_", "startprob_", "transmat_")


def params(m):
    return {f: np.ravel(getattr(m, f)).tolist() for f in FIELDS}


def spread(a, b, ll_a, ll_b):
    """Largest difference of two fits: parameters relative to max(1, largest |entry| of the field), log-likelihood to max(1, |ll|)."""
    worst = abs(ll_a - ll_b) / max(1.0, abs(ll_a))
    for f in FIELDS:
        u, v = np.ravel(np.asarray(a[f], dtype=float)), np.ravel(np.asarray(b[f], dtype=float))
        worst = max(worst, float(np.max(np.abs(u - v))) / max(1.0, float(np.max(np.abs(u)))))
    return worst


# ------------------------------------------------------------------------------------------------------------------- Viterbi
KLD_MODEL = dict(means=[0.04, 0.13], covars=[2e-4, 1.5e-3], start=[0.6, 0.4], trans=[[0.97, 0.03], [0.08, 0.92]])
# 600 k steps: log densities centred on 0 (variance 1 / (2 pi e)), so that the numpy path's running scores stay small and its own
# rounding stays far below MARGIN - with KLD-sized variances the scores reach 1e6, whose spacing (1e-10) is a tenth of MARGIN
FLAT_MODEL = dict(means=[-0.25, 0.25], covars=[0.0585, 0.0585], start=[0.5, 0.5], trans=[[0.95, 0.05], [0.05, 0.95]])


HARD_MODELS = {
    "forbidden": dict(means=[0.04, 0.13], covars=[2e-4, 1.5e-3], start=[0.6, 0.4], trans=[[1.0, 0.0], [0.08, 0.92]]),       # 0 -> 1 impossible
    "absorbing_start": dict(means=[0.04, 0.13], covars=[2e-4, 1.5e-3], start=[0.0, 1.0], trans=[[0.97, 0.03], [0.0, 1.0]]),  # 1 -> 0 impossible
    "symmetric": dict(means=[0.1, 0.1], covars=[1e-3, 1e-3], start=[0.5, 0.5], trans=[[0.5, 0.5], [0.5, 0.5]]),
}


def _two_regimes(rng, n, flip, model):
    st = np.cumsum(rng.random(n) < flip) % 2
    sd = np.sqrt(np.asarray(model["covars"]))
    mu = np.asarray(model["means"])
    return rng.normal(mu[st], sd[st])


def viterbi_case(name):
    """(x, seg_off, model dict)"""
    if name == "short_segments":
        rng = np.random.default_rng(201)
        lens = rng.integers(0, 40, 3000)
        model = KLD_MODEL
    elif name == "long_segment":
        rng = np.random.default_rng(202)
        lens = np.array([600000])
        model = FLAT_MODEL
    elif name == "cuts":
        rng = np.random.default_rng(203)
        V = VIT_STEPS
        lens = np.array([V, 2 * V, 1, V - 1, V + 1, 0, 3 * V, 3 * V + 1, 0, 2, 5 * V - 1, V, 0])
        model = KLD_MODEL
    elif name == "empty":
        rng = np.random.default_rng(204)
        lens = np.array([0, 0, 5, 0, 0, 1, 0])
        model = KLD_MODEL
    elif name in HARD_MODELS:
        # every segment length around a cut of the device's pieces, hard models: a transition that cannot happen (log 0) and
        # exact ties now CROSS cuts (hmm_vit_cuts' -inf and tie handling, hmm_vit_pieces' per-entry backpointers)
        rng = np.random.default_rng(205 + list(HARD_MODELS).index(name))
        V = VIT_STEPS
        lens = np.array([V - 1, V, V + 1, 2 * V + 1, 5 * V, 0])
        model = HARD_MODELS[name]
    else:
        raise KeyError(name)
    seg_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    x = _two_regimes(rng, int(seg_off[-1]), 0.02, KLD_MODEL if name in HARD_MODELS else model)
    return np.ascontiguousarray(x, dtype=np.float64), seg_off, model


VITERBI_CASES = ("short_segments", "long_segment", "cuts", "empty") + tuple(HARD_MODELS)
TIED = ("symmetric",)     # every decision an exact tie: no margin to demand; the path must be all zeros


def model_of(model, native, device=0):
    m = GaussianHMM2(native=native, device=device)
    m.means_, m.covars_ = np.array(model["means"], float), np.array(model["covars"], float)
    m.startprob_, m.transmat_ = np.array(model["start"], float), np.array(model["trans"], float)
    return m


def numpy_path_and_margin(m, x, count=None):
    """GaussianHMM2._predict_py, operation for operation, and the smallest |cand[0][j] - cand[1][j]| over every step and both
    target states j whose difference is FINITE, the final choice included (inf for sequences of no such decision).  A pair of
    -inf candidates is a tie to the lower state (as numpy.argmax decides it), one -inf candidate is decided by an infinite margin;
    `count` (a dict) receives how many decisions were finite, had one -inf candidate, or two."""
    if x.size == 0:
        return np.zeros(0, dtype=int), float("inf")
    b = m._loglik(x)
    with np.errstate(divide="ignore"):
        lt, ls = np.log(m.transmat_), np.log(m.startprob_)
    n = x.size
    score = ls + b[0]
    back = np.zeros((n, 2), dtype=int)
    margin = float("inf")
    tally = {"finite": 0, "one_neg_inf": 0, "two_neg_inf": 0}

    def decide(c0, c1):
        nonlocal margin
        for u, v in zip(np.atleast_1d(c0).tolist(), np.atleast_1d(c1).tolist()):
            ninf = (u == -np.inf) + (v == -np.inf)
            tally[("finite", "one_neg_inf", "two_neg_inf")[ninf]] += 1
            if ninf == 0:
                margin = min(margin, abs(u - v))
    for t in range(1, n):
        cand = score[:, None] + lt
        back[t] = cand.argmax(axis=0)
        decide(cand[0], cand[1])
        score = cand.max(axis=0) + b[t]
    decide(score[0], score[1])
    path = np.empty(n, dtype=int)
    path[-1] = int(score.argmax())
    for t in range(n - 1, 0, -1):
        path[t - 1] = back[t, path[t]]
    if count is not None:
        for k, v in tally.items():
            count[k] = count.get(k, 0) + v
    return path, margin


def numpy_states(model, x, seg_off, with_margin=False, count=None):
    """States of every segment by the numpy path (int8), and - on request - the smallest decision margin."""
    m = model_of(model, native=False)
    out = np.zeros(x.size, dtype=np.int8)
    margin = float("inf")
    for a, b in zip(seg_off[:-1].tolist(), seg_off[1:].tolist()):
        if with_margin:
            path, mg = numpy_path_and_margin(m, x[a:b], count)
            margin = min(margin, mg)
        else:
            path = m._predict_py(x[a:b])
        out[a:b] = path
    return (out, margin) if with_margin else out
