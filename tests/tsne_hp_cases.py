"""The cases of the extended-precision t-SNE pin (tests/test_tsne_hp_cpu.py, tests/test_gpu_tsne_edges.py): seeded inputs, the
comparison both tests use, and the float64 model whose distance from the oracle sets the allowed ratios.  TEST INFRASTRUCTURE.

The model is tests/tsne_oracle.py (`affinities`, `step(..., gram=False)`): float64 numpy with direct differences and numpy's
pairwise sums.  A model of the device's own order (strided per-thread sums, a xor butterfly per wave, the waves in order) was
judged not worth it: both are trees over short serial runs, and the allowed ratio is 8 x the model's worst over the whole case
set, per quantity, as tests/golden/hmm_gpu.json and hmm_estep.json do.  No figure here comes from a device.

tools/make_golden_tsne_hp.py writes tests/golden/tsne_hp.json and the arrays beside it from this module.
"""
import functools
import hashlib
import json
import os

import numpy as np

import tsne_oracle as TO
import tsne_oracle_hp as HP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLD, "tsne_hp.json")
DIR = os.path.join(GOLD, "tsne_hp")
FACTOR = 8
MARGIN = 1e-9               # every compared bisection decision is at least this far from flipping (H carries about 1e-13)
QUANTITIES = ("q", "dY", "iY", "Y", "cost")         # dY is measured for the model only: it decides which gains are compared
SAMPLED_ROWS = lambda n: [0, 1023, 1024, 4100, n - 2, n - 1]        # noqa: E731
CENTRE_ROWS = [0, 255, 256, 4095, 4096]


def golden():
    return json.load(open(JSON))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def blobs(n, f, seed):
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(4, f))
    return centres[rs.randint(0, 4, n)] + 0.3 * rs.normal(size=(n, f))


def perplexity_of(n):
    return min(20.0, max(1.5, n / 4.0))


# ---------------------------------------------------------------------------------------------------------- affinity cases
class Aff:
    """kind: plain | offset (X + 1e4) | cap_up (12 copies of row 0, perplexity 5) | cap_down (perplexity n > n - 1)."""

    def __init__(self, n, f, kind="plain", seed=None):
        self.n, self.f, self.kind = n, f, kind
        self.seed = SEEDS.get((n, f, kind), 1000 * n + f) if seed is None else seed
        self.id = "%s/n%d_f%d" % (kind, n, f)
        self.perplexity = {"cap_up": 5.0, "cap_down": float(n)}.get(kind, perplexity_of(n))
        # meant to sit on the cap (every row, or the copies): exempt from the margin on those rows
        down = kind == "cap_down" or (kind == "plain" and self.perplexity > n - 1)
        self.cap = "down" if down else "up" if kind == "cap_up" else None

    def X(self):
        X = blobs(self.n, self.f, self.seed)
        if self.kind == "offset":
            X = X + 1e4
        if self.kind == "cap_up":
            X[1:DUPS] = X[0]
        return X


DUPS = 12
# seeds: the first of 1000 n + f, + 1, ... at which every uncapped row's margins exceed MARGIN (the CPU test asserts it);
# only those that differ from 1000 n + f are listed
SEEDS = {(257, 5, "plain"): 257006, (1025, 1, "plain"): 1025002}
AFF = [Aff(n, 5) for n in (2, 3, 63, 64, 65, 1023, 1024, 1025)] + [Aff(n, f) for n in (65, 1025) for f in (1, 64)] + [
    Aff(65, 5, "offset"), Aff(65, 5, "cap_up"), Aff(2, 5, "cap_down"), Aff(65, 5, "cap_down")]
AFF_BY_ID = {c.id: c for c in AFF}
# recorded cases: the first seed from 0 (8192), 1000 (8193), 2049000 (2049) at which a float64 run of the bisection kept every
# row's margins above 1.1e-9 (a long-double run of one seed takes minutes); the record holds the long-double margins
RECORDED_TOTALS = {}            # filled by tools/make_golden_tsne_hp.py while it writes the record; otherwise read from the record
RECORDED = {"n8192_f5": (8192, 5, 2), "n8193_f5": (8193, 5, 1040), "n2049_f5": (2049, 5, 2049000)}      # id: (n, f, seed)


def outlier_X():
    """1024 ordinary rows and row 1024 at 1e200: that row's distances overflow, its sum P is 0."""
    X = blobs(1025, 5, 77)
    X[1024] = 1e200
    return X


@functools.lru_cache(maxsize=4)
def _oracle_aff(n, f, kind, seed):
    c = Aff(n, f, kind, seed)
    return HP.affinities(c.X(), c.perplexity)


def oracle_aff(c):
    return _oracle_aff(c.n, c.f, c.kind, c.seed)


def capped(c, o):
    """The rows that are meant to end at 50 tries."""
    rows = np.zeros(c.n, dtype=bool)
    if c.cap == "down":
        rows[:] = True
    elif c.cap == "up":
        rows[:DUPS] = True
    return rows


def margins(c, o):
    """(smallest | |Hdiff| - 1e-5 |, smallest |Hdiff|) over the rows that are not meant to sit on the cap (inf if none)."""
    keep = ~capped(c, o)
    return (float(o["m_tol"][keep].min()), float(o["m_sign"][keep].min())) if keep.any() else (float("inf"), float("inf"))


def check_aff(c, o, beta, tries, q, allowed, what="GPU"):
    """beta and tries equal to the oracle's, q symmetric and within allowed x unit; the cap cases' exact values.  Returns the
    worst q ratio."""
    assert tries.tolist() == o["tries"].tolist(), what
    assert np.array_equal(beta, o["beta"]), what
    cap = capped(c, o)
    if c.cap == "down":
        assert (tries == 50).all() and (beta == 2.0 ** -50).all()
    if c.cap == "up":
        assert (tries[cap] == 50).all() and (beta[cap] == 2.0 ** 50).all() and (tries[~cap] < 50).all()
        block = q[:DUPS, :DUPS][~np.eye(DUPS, dtype=bool)]
        assert (block == block[0]).all()                    # the copies' p are equal: exp(0) / 11, twice, over one total
        first = q[0, DUPS:]
        assert all(np.array_equal(q[i, DUPS:], first) for i in range(1, DUPS))      # p_j|i = 0 exactly: only p_i|j is left
        assert o["below_floor"][:DUPS, DUPS:].any()
    # where the unclamped value is below half the floor (the copies' p_j|i is exactly 0 there), q is exactly the floor; elsewhere
    # a copy's entry carries only beta_j's share in its unit
    assert (q[o["below_floor"]] == float(HP.Q_FLOOR)).all(), what
    assert np.array_equal(q, q.T), what
    r = HP.ratio(q, o["q"], o["u_q"])
    assert r <= allowed, (what, c.id, r, allowed)
    return r


def gram_q(X, beta):
    """q from given betas in float64 with the reference's Gram-form distances |a|^2 + |b|^2 - 2 a.b: what the kernel must not do."""
    s = np.sum(np.square(X), 1)
    D = np.add(np.add(-2 * np.dot(X, X.T), s).T, s)
    P = np.exp(-D * beta[:, None])
    np.fill_diagonal(P, 0.0)
    P = P / P.sum(axis=1)[:, None]
    P = P + P.T
    return np.maximum(P / P.sum(), float(HP.Q_FLOOR))


# ---------------------------------------------------------------------------------------------------------- step cases
class StepCase:
    """kind: plain | far (two groups 1e7 apart) | coincident (equal Y rows) | min_gain (gains 0.0124 / 0.0126 under x 0.8)."""

    def __init__(self, n, d, t, kind="plain", recorded=None):
        self.n, self.d, self.t, self.kind, self.recorded = n, d, t, kind, recorded
        self.id = "%s/n%d_d%d_t%d" % (kind, n, d, t)
        self.seed = 7 * n + d
        self.perplexity = perplexity_of(n)

    def aff(self):
        return Aff(self.n, 5)

    def X(self):
        return blobs(self.n, 5, RECORDED[self.recorded][2]) if self.recorded else self.aff().X()

    def state(self, q=None):
        """(Y, iY, gains): Y normal, iY of both signs with a tenth of its entries exactly 0, gains from {0.8, 1, 1.2, 2.2}."""
        rs = np.random.RandomState(self.seed + 100 * self.t)
        n, d = self.n, self.d
        Y = rs.randn(n, d)
        iY = 0.1 * rs.randn(n, d)
        iY[rs.rand(n, d) < 0.1] = 0.0
        gains = rs.choice([0.8, 1.0, 1.2, 2.2], (n, d))
        if self.kind == "far":
            Y[: n // 2, 0] += 1e7
        if self.kind == "coincident":
            Y[1:4] = Y[0]
            Y[6] = Y[5]
        if self.kind == "min_gain":         # iY takes the sign of the oracle's dY (which depends on neither iY nor gains): x 0.8
            dY = HP.step(Y, iY, gains, q, self.t)["dY"]
            iY = np.where(dY > 0, 0.05, -0.05)
            gains = np.where((np.arange(n * d).reshape(n, d) % 2) == 0, 0.0124, 0.0126)
        return Y, iY, gains


T_SWEEP = (0, 9, 19, 20, 99, 100, 101, 109)
STEPS = ([StepCase(67, d, 0) for d in (1, 2, 4, 5, 16, 17, 64)]
         + [StepCase(n, 2, 9) for n in (7, 8, 9, 15, 16, 17)]
         + [StepCase(n, 5, 9) for n in (2, 3, 256, 257)]
         + [StepCase(n, d, 109) for n in (255, 256, 257) for d in (2, 17)] + [StepCase(255, 5, 109)]
         + [StepCase(257, 17, 9), StepCase(513, 5, 109), StepCase(2049, 2, 9, recorded="n2049_f5")]
         + [StepCase(65, d, t) for d in (2, 5, 17) for t in T_SWEEP]
         + [StepCase(65, 2, 0, "far"), StepCase(65, 2, 9, "far"), StepCase(65, 5, 109, "far"), StepCase(65, 17, 9, "far")]
         + [StepCase(65, 2, 9, "coincident"), StepCase(65, 17, 0, "coincident")]
         + [StepCase(65, d, 20, "min_gain") for d in (2, 5, 17)])
# (2049, 2), (513, 5), (257, 17): 257 partials for tsne_sum; (512, 5): 256
STEPS.append(StepCase(512, 5, 9))
STEP_BY_ID = {c.id: c for c in STEPS}
assert len(STEP_BY_ID) == len(STEPS)


def recorded_arrays(rid):
    """(beta, tries, m_tol, m_sign) of a recorded case."""
    a = np.load(os.path.join(DIR, rid + "_rows.npy"))
    return a[:, 0].copy(), a[:, 1].astype(np.int32), a[:, 2].copy(), a[:, 3].copy()


@functools.lru_cache(maxsize=2)
def _recorded_q(rid):
    g = RECORDED_TOTALS[rid] if rid in RECORDED_TOTALS else golden()["recorded"][rid]
    n, f, seed = RECORDED[rid]
    beta, tries, _mt, _ms = recorded_arrays(rid)
    o = HP.affinities(blobs(n, f, seed), beta=beta, total=ld(g["total"]), rel_total=ld(g["rel_total"]))
    o["beta"], o["tries"] = beta, tries
    return o


def step_aff(c):
    """The oracle's affinities of a step case's X (computed, or from the recorded betas)."""
    return _recorded_q(c.recorded) if c.recorded else oracle_aff(c.aff())


def undecided(st, allowed_dY):
    return np.abs(st["dY"]) <= st["u_dY"] * allowed_dY


def skip_cap(entries):
    return max(2, entries // 1000)


def compare_step(c, st, Y, iY, gains, cost, allowed_dY):
    """{iY, Y, cost: worst ratio over the compared entries, "skipped": entries left out, "gains_differ": compared entries whose
    gains differ}.  An entry is left out when its gains differ and the sign of the oracle's dY is undecided."""
    skip = (gains != st["gains"]) & undecided(st, allowed_dY)
    out = {"iY": HP.ratio(iY, st["iY"], st["u_iY"], ~skip), "Y": HP.ratio(Y, st["Y"], st["u_Y"], ~skip), "skipped": int(skip.sum()),
           "gains_differ": int(np.count_nonzero((gains != st["gains"]) & ~skip))}
    if st["cost"] is not None:
        out["cost"] = HP.ratio(np.ravel(cost)[0], st["cost"], st["u_cost"])
    return out


def check_step(c, st, Y, iY, gains, cost, allowed, what="GPU"):
    """compare_step, asserted: gains equal on every compared entry, at most skip_cap entries left out, iY, Y and the cost (on
    cost iterations, and only then) within allowed x unit."""
    assert (st["cost"] is not None) == ((c.t + 1) % 10 == 0) and np.size(cost) == (st["cost"] is not None), (what, c.id)
    out = compare_step(c, st, Y, iY, gains, cost, allowed["dY"])
    assert out["gains_differ"] == 0 and out["skipped"] <= skip_cap(Y.size), (what, c.id, out)
    for k in ("iY", "Y", "cost"):
        assert out.get(k, 0.0) <= allowed[k], (what, c.id, k, out[k], allowed[k])
    return out


def model_step(c):
    """The float64 model on a step case: ({quantity: ratio}, oracle step, count of undecided entries is left to the caller)."""
    o = step_aff(c)
    X = c.X()
    if c.recorded:          # the model's q from the recorded betas (its own bisection is what the affinity cases measure)
        D = TO.sqdist(X)
        P = np.exp(-D * o["beta"][:, None])
        np.fill_diagonal(P, 0.0)
        P = P / P.sum(axis=1)[:, None]
        P = P + P.T
        q = np.maximum(P / P.sum(), TO.Q_FLOOR)
    else:
        q = TO.affinities(X, c.perplexity)[2]
    r = {"q": HP.ratio(q, o["q"], o["u_q"])}
    q_rel = float(np.max(np.abs(q.astype(HP.LD) - o["q"]) / o["q"]))
    Y, iY, gains = c.state(o["q"])
    st = HP.step(Y, iY, gains, o["q"], c.t, q_rel=q_rel)
    m = TO.step(Y, iY, gains, q, c.t, gram=False)
    r["dY"] = HP.ratio(m.dY, st["dY"], st["u_dY"])
    return r, st, m


# ---------------------------------------------------------------------------------------------------------- centring case
CENTRE_N, CENTRE_D = 4097, 64


def centre_inputs():
    """X: n equal points and a perplexity above n - 1, so every beta is 2^-50 and q_ij = 1 / (n (n - 1)) in closed form; Y0:
    column k around k, so a column mean taken from the wrong column is off by whole numbers."""
    rs = np.random.RandomState(4097)
    Y0 = np.arange(CENTRE_D, dtype=np.float64)[None, :] + 0.5 * rs.randn(CENTRE_N, CENTRE_D)
    return np.zeros((CENTRE_N, 1)), Y0, float(CENTRE_N)


def centre_unit(pre):
    """(mean, want, unit) of centring pre (long double): unit = eps (sum_i |pre_ik| / n + |mean_k| + |pre - mean|), the rounding
    of the column sum, of the division and of the subtraction (u_mean and u_Y of the oracle without the inherited u_pre)."""
    n = pre.shape[0]
    mean = HP._rowsum(pre.T) / n
    want = pre - mean
    return mean, want, HP.EPS * (HP._rowsum(np.abs(pre).T) / n + np.abs(mean) + np.abs(want))


def centre_model():
    """The worst ratio, in centre_unit, of a float64 centring of the centring case (Y0 plus a seeded iY of the step's size):
    column sums by numpy's pairwise sums along a contiguous axis, as the model's other sums.  Only + - /: the same everywhere."""
    _X, Y0, _p = centre_inputs()
    pre = Y0 + 1e-3 * np.random.RandomState(4098).randn(*Y0.shape)
    got = pre - np.ascontiguousarray(pre.T).sum(axis=1) / pre.shape[0]
    _mean, want, unit = centre_unit(pre.astype(HP.LD))
    return HP.ratio(got, want, unit)


def centre_q():
    return 1 / (HP.LD(CENTRE_N) * (CENTRE_N - 1))


def ld(pair):
    return HP.LD(pair[0]) + HP.LD(pair[1])


def pair(v):
    """A long double as two float64 (exact: 64 mantissa bits fit in 53 + 53)."""
    hi = float(v)
    return [hi, float(HP.LD(v) - HP.LD(hi))]


def mp_distances():
    """The oracle's distance from 50-digit arithmetic on three small cases (inputs from the generator alone: no exp or log)."""
    X = blobs(12, 3, 1)
    rs = np.random.RandomState(3)
    Y, iY = rs.randn(12, 2), 0.1 * rs.randn(12, 2)
    q = rs.rand(12, 12) ** 4
    q = q + q.T
    np.fill_diagonal(q, 0.0)
    q = np.maximum(q / q.sum(), float(HP.Q_FLOOR))
    return {"affinities_n12_f3": HP.distance_from_mp(X=X, perplexity=3.0),
            "step_n12_d2_t0": HP.distance_from_mp(Y=Y, iY=np.zeros_like(Y), gains=np.ones_like(Y), q=q, t=0),
            "step_n12_d2_t109": HP.distance_from_mp(Y=Y, iY=iY, gains=np.ones_like(Y), q=q, t=109)}
