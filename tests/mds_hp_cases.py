"""The cases of the extended-precision MDS pin (tests/test_mds_hp_cpu.py, tests/test_gpu_mds_edges.py): seeded inputs, the
comparison both tests use, the float64 model whose distance from the oracle sets the allowed ratios, and mutants of that model
that the comparison must refuse.  TEST INFRASTRUCTURE.

The model is tests/mds_oracle.py (`direct_D`, `step`, `stress`): float64 numpy with direct differences and numpy's own sums.
The allowed ratio per quantity (D, Y1, stress, v) is 8 x the model's worst over the whole case set, as tests/tsne_hp_cases.py,
tests/golden/hmm_gpu.json and hmm_estep.json do.  No figure here comes from a device.

Off the device the step cases take D from the oracle's dissimilarities rounded to float64 (the same bits everywhere); on the
device they take the device's own D.  The `settled` configurations are inputs made by mds_oracle_hp.settle from that D.

tools/make_golden_mds_hp.py writes tests/golden/mds_hp.json from this module.
"""
import functools
import hashlib
import json
import os

import numpy as np

import mds_oracle as MO
import mds_oracle_hp as HP

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JSON = os.path.join(GOLD, "mds_hp.json")
FACTOR = 8
QUANTITIES = ("D", "Y1", "stress", "v")     # v: relative to the oracle's v_T, in units of eps
F_STEP = 9                                  # width of the X behind every step, reduction and stop case
NEAR = 1e-7                                 # `pairs`: one pair of rows this far apart, below 1e-5 and not 0
SETTLE_STEPS = 50


def golden():
    return json.load(open(JSON))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def blobs(n, f, seed):
    rs = np.random.RandomState(seed)
    centres = rs.rand(3, f)
    return centres[rs.randint(0, 3, n)] + 0.05 * rs.rand(n, f)


# ---------------------------------------------------------------------------------------------------------- dissimilarities
class Dis:
    """kind: plain | offset (X + 1e4) | dups (a quarter of the rows copied) | close (a quarter of the rows 1e-9 from another)."""

    def __init__(self, n, f, kind):
        self.n, self.f, self.kind = n, f, kind
        self.id = "%s/n%d_f%d" % (kind, n, f)

    def X(self):
        n, f = self.n, self.f
        X = blobs(n, f, 1000 * n + f)
        q = max(1, n // 4)
        if self.kind == "offset":
            X = X + 1e4
        if self.kind == "dups":
            X[n - q:] = X[:q]
        if self.kind == "close":
            X[n - q:] = X[:q] + 1e-9 * np.random.RandomState(n + f).randn(q, f)
        return X


DIS_KINDS = ("plain", "offset", "dups", "close")
DIS_SHAPES = [(n, 9) for n in (2, 63, 64, 65, 129)] + [(65, f) for f in (1, 15, 16, 17, 33, 2772)]
DIS = [Dis(n, f, k) for n, f in DIS_SHAPES for k in DIS_KINDS]
DIS_BY_ID = {c.id: c for c in DIS}


def check_D(c, D, allowed, what="GPU"):
    """D symmetric with a zero diagonal, zero exactly where the oracle's is, within allowed x unit.  Returns the ratio."""
    o, u = HP.dissimilarities(c.X())
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0.0), (what, c.id)
    assert np.array_equal(D == 0.0, o == 0), (what, c.id)
    r = HP.ratio(D, o, u)
    assert r <= allowed, (what, c.id, r, allowed)
    return r


def gram_D(X):
    """Mutant: D in sklearn's Gram form."""
    s = (X * X).sum(axis=1)
    D = np.sqrt(np.maximum(s[:, None] + s[None, :] - 2.0 * (X @ X.T), 0.0))
    np.fill_diagonal(D, 0.0)
    return D


# ---------------------------------------------------------------------------------------------------------- step cases
class StepCase:
    """kind: plain (uniform start) | settled (50 updates on) | offset (plain + 1e4) | pairs (rows 0, 1 equal in X and in Y; rows
    2, 3 equal in Y only; row 5 within 1e-7 of row 4 in Y; at n < 6 only what fits) | collapsed (every row of Y equal)."""

    def __init__(self, n, d, kind="plain", rows=None):
        self.n, self.d, self.kind = n, d, kind
        self.rows = rows                    # Y1 is compared on these rows only (the reduction cases)
        self.id = "%s/n%d_d%d" % (kind, n, d)

    def X(self):
        X = blobs(self.n, F_STEP, 7 * self.n + self.d)
        if self.kind == "pairs" and self.n >= 4:
            X[1] = X[0]
        return X

    def D0(self):
        return _D0(self.n, self.d, self.kind == "pairs")

    def Y(self):
        return _Y(self.n, self.d, self.kind).copy()


@functools.lru_cache(maxsize=None)
def _D0(n, d, pairs):
    D = HP.dissimilarities(StepCase(n, d, "pairs" if pairs else "plain").X())[0].astype(np.float64)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def _Y(n, d, kind):
    Y = np.random.RandomState(31 * n + d).uniform(size=(n, d))
    if kind == "settled":
        Y = HP.settle(Y, _D0(n, d, False), SETTLE_STEPS)
    if kind == "offset":
        Y = Y + 1e4
    if kind == "pairs":
        Y[1] = Y[0]
        if n >= 4:
            Y[3] = Y[2]
        if n >= 6:
            Y[5] = Y[4]
            Y[5, 0] += NEAR
    if kind == "collapsed":
        Y[:] = Y[0]
    Y.setflags(write=False)
    return Y


STEP_SHAPES = sorted({(n, d) for d in (1, 2, 4, 5, 16, 17, 64) for n in (9, 257)}
                     | {(n, d) for d in (2, 5, 17) for n in (2, 7, 8, 9, 255, 256, 257, 513)})
STEPS = ([StepCase(n, d, k) for n, d in STEP_SHAPES for k in ("plain", "settled")]
         + [StepCase(n, d, k) for n, d in STEP_SHAPES if d in (2, 5, 17) for k in ("offset", "pairs", "collapsed")])
REDUCTION_ROWS = lambda n: sorted({0, 255, 256, n - 2, n - 1} & set(range(n)))      # noqa: E731
REDUCTIONS = [StepCase(n, d, "plain", rows=REDUCTION_ROWS(n))
              for n, d in ((2048, 2), (2049, 2), (512, 5), (513, 5), (256, 17), (257, 17))]
for _c in REDUCTIONS:
    _c.id = "parts/n%d_d%d" % (_c.n, _c.d)
STEP_BY_ID = {c.id: c for c in STEPS + REDUCTIONS}
assert len(STEP_BY_ID) == len(STEPS) + len(REDUCTIONS)


def compare_step(c, D, Y, Y1, s1):
    """{Y1, stress}: Y1 against the oracle's step from Y (on c.rows), s1 against the oracle's stress of Y1 itself."""
    o = HP.step(Y, D, rows=c.rows, sums=False)
    got = Y1 if c.rows is None else Y1[c.rows]
    o1 = HP.step(Y1, D, guttman=False)
    return {"Y1": HP.ratio(got, o["Y1"], o["u_Y1"]), "stress": HP.ratio(s1, o1["stress"], o1["u_stress"])}, o, o1


def check_step(c, D, Y, Y1, s1, allowed, what="GPU"):
    r, o, o1 = compare_step(c, D, Y, Y1, s1)
    for k in ("Y1", "stress"):
        assert r[k] <= allowed[k], (what, c.id, k, r[k], allowed[k])
    if c.kind == "collapsed":
        assert not Y1.any() and (o["u_Y1"] == 0).all() and o1["sumsq"] == 0, (what, c.id)
    return r


def model_step(c, step=MO.step, stress=MO.stress):
    """The float64 model (or a mutant of it) on a step case: (Y1, the stress of Y1)."""
    D, Y = c.D0(), c.Y()
    Y1 = step(Y, D)
    return Y1, stress(Y1, D)[0]


# mutants of the step, all float64
def gram_step(Y, D):
    """sklearn's form: Gram-form configuration distances and (1 / n) B Y."""
    n = Y.shape[0]
    s = (Y * Y).sum(axis=1)
    dist = np.sqrt(np.maximum(s[:, None] + s[None, :] - 2.0 * (Y @ Y.T), 0.0))
    np.fill_diagonal(dist, 0.0)
    dist[dist == 0] = MO.ZERO_DIST
    B = -(D / dist)
    B[np.arange(n), np.arange(n)] += (D / dist).sum(axis=1)
    return (B @ Y) / n


def _step_with(Y, D, rule, cols=None):
    n = Y.shape[0]
    cols = n if cols is None else cols
    diff = Y[:, None, :] - Y[None, :cols, :]
    dist = np.sqrt((diff * diff).sum(-1))
    ratio = D[:, :cols] / np.where(rule(dist), MO.ZERO_DIST, dist)
    ratio[np.arange(cols), np.arange(cols)] = 0.0
    return np.einsum("ij,ijk->ik", ratio, diff) * (1.0 / n)


def drop_last_step(Y, D):
    return _step_with(Y, D, lambda dist: dist == 0.0, cols=Y.shape[0] - 1)


def less_than_rule_step(Y, D):
    return _step_with(Y, D, lambda dist: dist < MO.ZERO_DIST)


def replaced_stress(Y, D):
    """The stress taken from the distances after their zeros were replaced by 1e-5."""
    dist = MO.distances(Y)
    dist[dist == 0] = MO.ZERO_DIST          # the diagonal too, as sklearn's replacement does
    return float(((dist - D) ** 2).sum() / 2), float((dist ** 2).sum() / 2)


def distD_sums(Y, D):
    """sum dist^2 replaced by sum dist D."""
    dist = MO.distances(Y)
    return float(((dist - D) ** 2).sum() / 2), float((dist * D).sum() / 2)


# ---------------------------------------------------------------------------------------------------------- stop rule
class StopCase:
    def __init__(self, n, d, T):
        self.n, self.d, self.T = n, d, T
        self.id = "stop/n%d_d%d_T%d" % (n, d, T)
        self.seed = STOP_SEEDS[(n, d)]

    def X(self):
        return blobs(self.n, F_STEP, self.seed)

    def D0(self):
        return _stop_D0(self.n, self.seed)

    def Y0(self):
        return np.random.RandomState(self.seed + 1).uniform(size=(self.n, self.d))


# the first seed from 1000 n + d at which v_1 .. v_{T-1} > v_T (1 + 2 delta) for T = 1, 2, 3 (the CPU test asserts it)
STOP_SEEDS = {(65, 2): 65006, (257, 5): 257006}
STOP_ITERS = 5                              # iterations of the oracle's run behind the recorded v_t
STOPS = [StopCase(n, d, T) for n, d in sorted(STOP_SEEDS) for T in (1, 2, 3)]
STOP_BY_ID = {c.id: c for c in STOPS}


@functools.lru_cache(maxsize=None)
def _stop_D0(n, seed):
    return HP.dissimilarities(blobs(n, F_STEP, seed))[0].astype(np.float64)


@functools.lru_cache(maxsize=None)
def _oracle_run(n, d, seed):
    c = StopCase(n, d, 1)
    return HP.run(c.Y0(), c.D0(), STOP_ITERS, 0.0)


def oracle_run(c):
    return _oracle_run(c.n, c.d, c.seed)


def model_run(Y0, D, max_iter, eps, step=MO.step, sums=MO.stress):
    """State::run in float64 with the model's step and sums: (Y, stress, n_iter, trace, v)."""
    cur = step(Y0, D)
    old, it, trace, vs = 0.0, 0, [], [float("nan")]
    while True:
        last = it + 1 >= max_iter
        s, half_sq = sums(cur, D)
        trace.append(s)
        if it > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                vs.append(np.float64(old - s) / np.float64(half_sq))
            if vs[-1] < eps:
                break
        old = s
        if last:
            break
        cur = step(cur, D)
        it += 1
    return cur, s, it + 1, trace, vs


def v_error(v, want):
    """|v - want| / want in units of eps."""
    return float(abs(HP.LD(v) - want) / want / HP.EPS)


def margin(v, T):
    """min over t < T of v_t / v_T - 1 (inf at T = 1): the condition is margin > 2 delta."""
    return min([float(v[t] / v[T] - 1) for t in range(1, T)] + [float("inf")])


def check_stop(c, o, delta, runner, allowed_Y1, what="GPU"):
    """runner(Y0, max_iter, eps) -> (Y, stress, n_iter, trace), against the oracle's run o (from the same D): stops after T + 1
    passes with eps just above v_T, after T + 2 with eps just below.  Returns the ratio of Y to X_{T+1}."""
    T, v = c.T, o["v"]
    assert margin(v, T) > 2 * delta and v[T] > 0, (what, c.id)
    Y, s, it, trace = runner(c.Y0(), T + 2, float(v[T] * (1 + HP.LD(delta))))
    assert it == T + 1 and len(trace) == T + 1 and trace[-1] == s, (what, c.id, it, T)
    r = HP.ratio(Y, o["states"][T], o["u_states"][T])
    assert r <= allowed_Y1, (what, c.id, r, allowed_Y1)
    _Y, _s, it2, trace2 = runner(c.Y0(), T + 2, float(v[T] * (1 - HP.LD(delta))))
    assert it2 == T + 2 and len(trace2) == T + 2, (what, c.id, it2, T)
    assert list(trace2[:T + 1]) == list(trace), (what, c.id)
    return r


DRIVER_SHAPES = ((65, 2), (257, 5))


def check_driver(n, d, D, runner, allowed, what="GPU"):
    """The driver's edges on the plain and collapsed configurations of a step shape, runner(Y0, max_iter, eps) as in check_stop:
    max_iter = 1 returns X_1 after one pass; max_iter = 2 with eps = 1e300 stops at it = 1 with X_2; an all-coincident start
    with eps = 0 never stops (0 / 0 < 0 is false) and repeats one stress bit for bit.  Returns the worst ratio of Y."""
    Y0 = StepCase(n, d).Y()
    Y, s, it, trace = runner(Y0, 1, 0.0)
    o = HP.run(Y0, D, 2, 1e300)
    assert it == 1 and len(trace) == 1 and trace[0] == s, (what, n, d)
    r1 = HP.ratio(Y, o["states"][0], o["u_states"][0])
    o1 = HP.step(Y, D, guttman=False)
    assert HP.ratio(s, o1["stress"], o1["u_stress"]) <= allowed["stress"], (what, n, d)
    Y, s, it, trace = runner(Y0, 2, 1e300)
    assert o["n_iter"] == 2 and it == 2 and len(trace) == 2 and trace[1] == s, (what, n, d, it)
    r2 = HP.ratio(Y, o["states"][1], o["u_states"][1])
    assert max(r1, r2) <= allowed["Y1"], (what, n, d, r1, r2)
    Yc = StepCase(n, d, "collapsed").Y()
    Y, s, it, trace = runner(Yc, 4, 0.0)
    assert it == 4 and len(trace) == 4 and len({float(t).hex() for t in trace}) == 1 and not np.asarray(Y).any(), (what, n, d, it)
    oc = HP.step(Yc, D, guttman=False)
    assert oc["sumsq"] == 0 and HP.ratio(s, oc["stress"], oc["u_stress"]) <= allowed["stress"], (what, n, d)
    return max(r1, r2)


# ---------------------------------------------------------------------------------------------------------- mutants
def _dis_ratio(cid, form):
    c = DIS_BY_ID[cid]
    o, u = HP.dissimilarities(c.X())
    return HP.ratio(form(c.X()), o, u)


def _step_ratio(cid, quantity, **kw):
    c = STEP_BY_ID[cid]
    Y1, s1 = model_step(c, **kw)
    return compare_step(c, c.D0(), c.Y(), Y1, s1)[0][quantity]


def _v_ratio(cid):
    c = STOP_BY_ID[cid]
    o = oracle_run(c)
    vs = model_run(c.Y0(), c.D0(), STOP_ITERS, 0.0, sums=distD_sums)[4]
    return v_error(vs[c.T], o["v"][c.T])


# name: (what it does, [(case, quantity, ratio of the mutant there)])
MUTANTS = {
    "gram_dist": ("Gram-form configuration distances and (1 / n) B Y",
                  [("offset/n257_d2", "Y1", lambda: _step_ratio("offset/n257_d2", "Y1", step=gram_step)),
                   ("offset/n9_d17", "Y1", lambda: _step_ratio("offset/n9_d17", "Y1", step=gram_step))]),
    "gram_D": ("Gram-form D",
               [("offset/n65_f9", "D", lambda: _dis_ratio("offset/n65_f9", gram_D)),
                ("close/n65_f9", "D", lambda: _dis_ratio("close/n65_f9", gram_D))]),
    "replaced_stress": ("stress taken from the 1e-5-replaced distances",
                        [("pairs/n257_d5", "stress", lambda: _step_ratio("pairs/n257_d5", "stress", stress=replaced_stress)),
                         ("collapsed/n9_d2", "stress", lambda: _step_ratio("collapsed/n9_d2", "stress", stress=replaced_stress))]),
    "drop_last": ("last column j = n - 1 dropped from the Guttman sum",
                  [("plain/n257_d2", "Y1", lambda: _step_ratio("plain/n257_d2", "Y1", step=drop_last_step)),
                   ("settled/n513_d17", "Y1", lambda: _step_ratio("settled/n513_d17", "Y1", step=drop_last_step))]),
    "less_than_rule": ("the 1e-5 rule applied at dist < 1e-5 instead of dist == 0",
                       [("pairs/n9_d2", "Y1", lambda: _step_ratio("pairs/n9_d2", "Y1", step=less_than_rule_step)),
                        ("pairs/n513_d17", "Y1", lambda: _step_ratio("pairs/n513_d17", "Y1", step=less_than_rule_step))]),
    "sumsq_dist_D": ("sum dist^2 of the stop rule replaced by sum dist D",
                     [("stop/n65_d2_T1", "v", lambda: _v_ratio("stop/n65_d2_T1")),
                      ("stop/n257_d5_T3", "v", lambda: _v_ratio("stop/n257_d5_T3"))]),
}


# ---------------------------------------------------------------------------------------------------------- the record
def measure():
    """Everything tests/golden/mds_hp.json holds but the mpmath distances, measured from the model: the document."""
    doc = {"factor": FACTOR, "unit_eps": 2.0 ** -52, "quantities": list(QUANTITIES),
           "model": "tests/mds_oracle.py: direct_D, step, stress; float64 numpy, direct differences, numpy's own sums"}
    worst = {q: {"ratio": 0.0, "case": None} for q in QUANTITIES}

    def note(q, r, cid):
        if r > worst[q]["ratio"]:
            worst[q] = {"ratio": r, "case": cid}

    doc["dissimilarities"] = {}
    for c in DIS:
        X = c.X()
        o, u = HP.dissimilarities(X)
        r = HP.ratio(MO.direct_D(X), o, u)
        doc["dissimilarities"][c.id] = {"X": sha(X), "zeros": int((o == 0).sum()), "ratio": r}
        note("D", r, c.id)
    doc["steps"] = {}
    for c in STEPS + REDUCTIONS:
        Y1, s1 = model_step(c)
        r = compare_step(c, c.D0(), c.Y(), Y1, s1)[0]
        doc["steps"][c.id] = {"X": sha(c.X()), "D": sha(c.D0()), "Y": sha(c.Y()), "ratios": r}
        note("Y1", r["Y1"], c.id)
        note("stress", r["stress"], c.id)
    doc["stops"] = {}
    for c in STOPS:
        o = oracle_run(c)
        Y, _s, _it, _tr, vs = model_run(c.Y0(), c.D0(), c.T + 1, 0.0)
        r = {"v": v_error(vs[c.T], o["v"][c.T]), "Y1": HP.ratio(Y, o["states"][c.T], o["u_states"][c.T])}
        doc["stops"][c.id] = {"seed": c.seed, "X": sha(c.X()), "D": sha(c.D0()), "Y0": sha(c.Y0()), "T": c.T,
                              "v": [float(x) for x in o["v"][1:]], "fall": float(1 - o["trace"][c.T] / o["trace"][c.T - 1]),
                              "margin": margin(o["v"], c.T) if c.T > 1 else None, "ratios": r}
        note("v", r["v"], c.id)
        note("Y1", r["Y1"], c.id)
    doc["worst"] = worst
    doc["allowed"] = {q: FACTOR * worst[q]["ratio"] for q in QUANTITIES}
    doc["delta"] = doc["allowed"]["v"] * 2.0 ** -52
    doc["mutants"] = {}
    for name, (what, sites) in MUTANTS.items():
        rec = []
        for cid, q, f in sites:
            r = f()
            rec.append({"case": cid, "quantity": q, "ratio": r, "over_allowed": r / doc["allowed"][q]})
        doc["mutants"][name] = {"what": what, "fails": rec}
    return doc


def mp_distances():
    """The oracle's distance from 50-digit arithmetic on three small cases: one D, one step (with a coincident pair), and the
    stress of a nearly settled configuration."""
    X = blobs(12, 3, 1)
    D = HP.dissimilarities(X)[0].astype(np.float64)
    Y = np.random.RandomState(3).uniform(size=(12, 2))
    Y[1] = Y[0]
    return {"D_n12_f3": HP.distance_from_mp(X=X), "step_n12_d2": HP.distance_from_mp(Y=Y, D=D),
            "settled_n12_d2": HP.distance_from_mp(Y=HP.settle(Y, D, SETTLE_STEPS), D=D)}
