"""Cases, reference access and the comparison routines of the tests of the HMM's deterministic start and first EM rounds (shared by
tools/make_golden_hmm_start.py, tests/test_hmm_start_cpu.py and tests/test_gpu_hmm_start.py).  Test infrastructure only.

START cases: every family at every size at which either layout of the start changes (tests/hmm_start_model.py) - the device's
chunk count C = clamp(n / 256, 1, 1024) goes 1 -> 2 at 512, 2 -> 3 at 768, reaches its cap at 262144, and 262144 + 1023 interleaves
chunks of 256 and 257 windows; the host's assignment is cut at n / 4096, 2 pieces from 8192, 256 from 1048576.  Families:
  regimes     two-regime draws of the KLD-like model (hmm_gpu_cases._two_regimes), clipped at 1e-4;
  overlap     an 85 : 15 mixture of N(0.05, 0.02) and N(0.10, 0.04): 2-means creeps, 20 rounds and more from 255 windows on;
  edges0..5   1000 +- 0.001 draws inside 1000 +- 0.0018 with ONE global minimum (1000 - 0.002) and ONE global maximum (1000 + 0.0025)
              at (min, max) = (0, n - 1), (n - 1, 0), (last window of a device chunk, first of the next), (first window of the
              host's next piece, last of a piece), (offsets 255, 256 of the device's LAST chunk), (offsets 256, 255 of the first
              chunk).  At this offset round 1 already meets the stop rule, so the start's means ARE the two extremes: 2-means run to
              a partition that no longer changes forgets the extremes it started from (measured: with 0.001 and 0.5 among KLD-like
              draws a maximum lost with the last chunk changed nothing below the cap), these inputs cannot;
  ties        dyadic values k / 1024, mirror images about 1 / 2 (every v has its 1 - v, so both centres lie equally far from 1 / 2
              whichever takes the ties), minimum 0, maximum 1, and windows at exactly (min + max) / 2 = 1 / 2 on the sequence's ends
              and on both layouts' chunk bounds.  Every sum is exact, so round 1's ties are ties in any arithmetic; sending them to
              centre 0 or to centre 1 gives two DIFFERENT stable partitions;
  constant    all windows 0.1;      two_values  0.03 and 0.15 only;
  offset      1000 +- 0.001 (a one-pass variance loses every digit);      negative    the regimes' draws minus 0.1 (both signs).
ROUND cases: `regimes` and `cuts` of tests/hmm_estep_cases.py (its KLD-like model's draws; outliers of 2.5 and -1.5 on the device
E step's cuts) at every size of E.SMALL and E.LARGE, fitted FROM THE START for one and for three rounds.  Both carry outliers, and
2-means from the extremes gives an outlier a centre of its own: state 1 is then the outliers alone, its mean never moves, and an
M step that took its covariance sums about the OLD means passed on every such case of more than 33 windows (measured with the
float64 model).  `plain` is the same draw without outliers: the start separates the two regimes and every round moves both means.
Inputs are regenerated from their seeds and their sha256 recorded.  References are long double (tests/hmm_oracle_hp.py): recomputed
at test time for the small sizes, recorded as (high, low) pairs of doubles for the large ones - the comparison is made in long
double, so no rounding of the reference enters it.
"""
import functools
import json
import os

import numpy as np

import hmm_estep_cases as E
import hmm_gpu_cases as H
import hmm_start_model as SM

LD = np.longdouble
JSON = os.path.join(E.GOLD, "hmm_start.json")
FACTOR = H.FACTOR          # 8
ORACLE_MARGIN = E.ORACLE_MARGIN      # 16
STOP_MARGIN = 1e-3         # every 2-means round's shift is at least this share of its stop threshold away from it
MIN_COVAR, COVARS_PRIOR = 1e-3, 1e-2      # GaussianHMM2's defaults, which every fit here uses

DEVICE_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 767, 768, 769, 262143, 262144, 262145, 262144 + 1023)
HOST_SIZES = (4095, 4096, 4097, 8191, 8192, 8193, 1048575, 1048576, 1048577)
SIZES = tuple(sorted(DEVICE_SIZES + HOST_SIZES))
SMALL = tuple(n for n in SIZES if n <= 8193)
LARGE = tuple(n for n in SIZES if n > 8193)
FAMILIES = ("regimes", "overlap", "edges0", "edges1", "edges2", "edges3", "edges4", "edges5", "ties", "constant", "two_values",
            "offset", "negative")
EDGE_MIN, EDGE_MAX = 1000.0 - 2e-3, 1000.0 + 2.5e-3      # the one minimum and the one maximum of the edges families
SLOW_FROM = 255           # `overlap` needs SLOW_ROUNDS rounds of 2-means from this size on
SLOW_ROUNDS = 20
# a case that failed a condition on the inputs (assignment margin, stop-rule margin, `overlap`'s round count) was given another seed
RESEED = {("regimes", 263167): 1,      # (round 1 decided a window by 6.1e-10 of the centre distance)
          # `overlap` below 4097 windows: the first seed whose draw needs SLOW_ROUNDS rounds
          ("overlap", 255): 18, ("overlap", 256): 38, ("overlap", 257): 44, ("overlap", 511): 22, ("overlap", 512): 1, ("overlap", 513): 23,
          ("overlap", 767): 5, ("overlap", 768): 9, ("overlap", 769): 6, ("overlap", 4095): 1, ("overlap", 4096): 1}

ROUND_MODEL = "kld"
ROUND_FAMILIES = E.FAMILIES + ("plain",)
ROUND_SIZES = E.SMALL + E.LARGE
ROUNDS = (1, 3)
START_Q = ("start_means", "start_covars")
ROUND_Q = ("fit1_params", "fit1_loglik", "fit3_params", "fit3_loglik")
QUANTITIES = START_Q + ROUND_Q
FORMS = ("numpy", "model", "host")      # the numpy specification, the float64 model in the device's layout, the host-native library


def start_id(family, n):
    return "%s-%d" % (family, n)


def round_id(family, n):
    return "rounds-%s-%d" % (family, n)


def start_cases(sizes=SIZES):
    return [(f, n) for f in FAMILIES for n in sizes]


def round_cases(sizes=ROUND_SIZES):
    return [(f, n) for f in ROUND_FAMILIES for n in sizes]


def _distinct(pmin, pmax, n):
    pmin, pmax = min(max(pmin, 0), n - 1), min(max(pmax, 0), n - 1)
    if pmin == pmax:
        pmin = pmax - 1 if pmax > 0 else pmax + 1
    return pmin, pmax


def edge_positions(k, n):
    """(window of the minimum, window of the maximum) of family edges<k>; n >= 2."""
    C, P = SM.parts_of(n), SM.host_parts_of(n)
    D, Hc = SM.bounds(n, C), SM.bounds(n, P)
    dc = int(D[C // 2]) if C >= 2 else n // 2
    hc = int(Hc[P // 2]) if P >= 2 else n // 2
    last = int(D[C - 1])
    return _distinct(*[(0, n - 1), (n - 1, 0), (dc - 1, dc), (hc, hc - 1), (last + 255, last + 256), (256, 255)][k], n)


def tie_positions(n):
    C, P = SM.parts_of(n), SM.host_parts_of(n)
    D, Hc = SM.bounds(n, C), SM.bounds(n, P)
    t = {0, n - 1, n // 2 - 1, n // 2, 255, 256, int(D[C - 1]) - 1, int(D[C - 1]), int(D[C // 2]) - 1, int(D[C // 2]), int(Hc[P // 2]) - 1, int(Hc[P // 2])}
    return sorted(p for p in t if 0 <= p < n)


def start_input(family, n):
    rng = np.random.default_rng([FAMILIES.index(family), n, 20262, RESEED.get((family, n), 0)])
    if family in ("regimes", "negative"):
        x = H._two_regimes(rng, n, 0.02, H.KLD_MODEL).clip(1e-4, None) - (0.1 if family == "negative" else 0.0)
    elif family == "overlap":
        x = np.where(rng.random(n) < 0.85, rng.normal(0.05, 0.02, n), rng.normal(0.10, 0.04, n))
    elif family.startswith("edges"):
        st = np.cumsum(rng.random(n) < 0.02) % 2
        x = 1000.0 + rng.normal(np.where(st == 0, -1e-3, 1e-3), 3e-4).clip(-1.8e-3, 1.8e-3)
        if n == 1:
            x[0] = EDGE_MAX
        else:
            pmin, pmax = edge_positions(int(family[5:]), n)
            x[pmin], x[pmax] = EDGE_MIN, EDGE_MAX
    elif family == "ties":
        if n < 8:
            x = np.array([0.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5][:n]) if n > 1 else np.array([0.5])
        else:
            x = np.full(n, 0.5)
            ties = set(tie_positions(n))
            rest = rng.permutation(np.array([p for p in range(n) if p not in ties], dtype=np.int64))
            half = rest.size // 2              # (an odd window out stays at 1 / 2)
            v = rng.integers(1, 257, half) / 1024.0
            v[0] = 0.0
            x[rest[:half]], x[rest[half:2 * half]] = v, 1.0 - v
    elif family == "constant":
        x = np.full(n, 0.1)
    elif family == "two_values":
        x = np.where(np.cumsum(rng.random(n) < 0.02) % 2 == 0, 0.03, 0.15)
        x[0], x[n - 1] = 0.03, (0.15 if n > 1 else 0.03)
    elif family == "offset":
        st = np.cumsum(rng.random(n) < 0.02) % 2
        x = 1000.0 + rng.normal(np.where(st == 0, -1e-3, 1e-3), 3e-4)
    else:
        raise KeyError(family)
    return np.ascontiguousarray(x, dtype=np.float64)


def round_input(family, n):
    if family == "plain":
        rng = np.random.default_rng([n, 20263, RESEED.get((family, n), 0)])
        return np.ascontiguousarray(H._two_regimes(rng, n, E.FLIP, E.MODELS[ROUND_MODEL]).clip(1e-4, None), dtype=np.float64)
    return E.case_input(ROUND_MODEL, family, n)


# ------------------------------------------------------------------------------------------------------------ long doubles as data
def split(v):
    """A long double as [high, low] doubles (exact: 64 bits fit in 53 + 53)."""
    hi = float(v)
    return [hi, float(LD(v) - LD(hi))]


def join(p):
    return LD(p[0]) + LD(p[1])


def ref_of_start(st):
    return {"means": [LD(v) for v in st["means"]], "covar": LD(st["covar"]), "rounds": int(st["rounds"])}


def ref_of_rounds(fr):
    """fit_rounds' list -> {r: {"means_": [..], .., "loglik": ll}} for r in ROUNDS, long doubles."""
    out = {}
    for r in ROUNDS:
        m, ll = fr[r - 1]
        out[r] = {"means_": [LD(v) for v in m["means"]], "covars_": [LD(v) for v in m["covars"]], "startprob_": [LD(v) for v in m["start"]],
                  "transmat_": [LD(v) for row in m["trans"] for v in row], "loglik": LD(ll)}
    return out


def pack_start(ref):
    return {"means": [split(v) for v in ref["means"]], "covar": split(ref["covar"])}


def pack_rounds(ref):
    return {str(r): {f: ([split(v) for v in d[f]] if f != "loglik" else split(d[f])) for f in d} for r, d in ref.items()}


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(JSON))


@functools.lru_cache(maxsize=None)
def start_account(family, n):
    """The oracle's whole account of a small case (hmm_oracle_hp.start), computed once."""
    import hmm_oracle_hp as O
    return O.start(start_input(family, n), MIN_COVAR)


@functools.lru_cache(maxsize=None)
def start_reference(family, n):
    if n in LARGE:
        c = golden()["start_cases"][start_id(family, n)]
        return {"means": [join(p) for p in c["oracle"]["means"]], "covar": join(c["oracle"]["covar"]), "rounds": c["rounds"]}
    return ref_of_start(start_account(family, n))


@functools.lru_cache(maxsize=None)
def round_reference(family, n):
    if n in E.LARGE:
        c = golden()["round_cases"][round_id(family, n)]["oracle"]
        return {int(r): {f: ([join(p) for p in d[f]] if f != "loglik" else join(d[f])) for f in d} for r, d in c.items()}
    import hmm_oracle_hp as O
    fr = O.fit_rounds(round_input(family, n), max(ROUNDS), MIN_COVAR, COVARS_PRIOR)
    ref = ref_of_rounds(fr)
    ref["lls"] = [ll for _m, ll in fr]      # (every round's, for round_conditions)
    return ref


# ------------------------------------------------------------------------------------------------------------------ comparisons
def _rel(got, ref):
    """Largest |got - ref| / max(1, |ref|) over the entries, in long double; anything non-finite is an infinite error."""
    worst = 0.0
    for g, r in zip(np.ravel(np.asarray(got, dtype=np.float64)).tolist(), ref):
        d = abs(LD(g) - r) / max(LD(1), abs(r))
        worst = max(worst, float(d) if np.isfinite(d) else float("inf"))
    return worst


def start_errors(got, ref):
    """got = (means [2], covars [2] or one covar): {quantity: error}, relative to max(1, |value|)."""
    means, covars = got
    return {"start_means": _rel(means, ref["means"]), "start_covars": _rel(covars, [ref["covar"]] * np.size(covars))}


def round_errors(r, got, ref):
    """got = (parameters as H.params gives them, loglik) after r rounds; errors as H.spread measures them: a field's largest
    difference relative to max(1, its largest |entry|), the log-likelihood's to max(1, |ll|) - against the long-double reference."""
    par, ll = got
    worst = 0.0
    for f in H.FIELDS:
        scale = max(LD(1), max(abs(v) for v in ref[r][f]))
        for g, v in zip(np.ravel(np.asarray(par[f], dtype=np.float64)).tolist(), ref[r][f]):
            d = abs(LD(g) - v) / scale
            worst = max(worst, float(d) if np.isfinite(d) else float("inf"))
    d = abs(LD(ll) - ref[r]["loglik"]) / max(LD(1), abs(ref[r]["loglik"]))
    return {"fit%d_params" % r: worst, "fit%d_loglik" % r: float(d) if np.isfinite(d) else float("inf")}


def check_start(family, n, got, tol=None, what="device"):
    tol = tol or golden()["tolerance"]
    e = start_errors(got, start_reference(family, n))
    msg = "%s %s (C = %d, host pieces %d): start means %.3g (allowed %.3g), start covars %.3g (%.3g)" % (
        what, start_id(family, n), SM.parts_of(n), SM.host_parts_of(n), e["start_means"], tol["start_means"], e["start_covars"],
        tol["start_covars"])
    assert all(e[q] <= tol[q] for q in START_Q), msg
    return e, msg


def check_rounds(family, n, r, got, tol=None, what="device"):
    tol = tol or golden()["tolerance"]
    e = round_errors(r, got, round_reference(family, n))
    msg = "%s %s after %d round(s): %s" % (what, round_id(family, n), r, ", ".join("%s %.3g (allowed %.3g)" % (q, e[q], tol[q]) for q in e))
    assert all(e[q] <= tol[q] for q in e), msg
    return e, msg


def check_device_rounds(family, n, r, got, what="device"):
    """The round comparison of the GPU test: the tolerance of all three forms, which the numpy specification sets - its log-space
    recursion loses digits with n (2.7e-8 on the one-round parameters at 524288 windows) -, and the bound of the same making from
    the two forms that work in scaled space as the device does, the float64 model of its layout and the host-native library
    (3e-14 .. 2.5e-12)."""
    e, msg = check_rounds(family, n, r, got, what=what)
    check_rounds(family, n, r, got, tol=golden()["tolerance_scaled_forms"], what=what + ", scaled-space bound,")
    return e, msg


# --------------------------------------------------------------------------------------------- conditions on the inputs (oracle only)
def start_conditions(family, n, st):
    """Assert what the inputs must meet, on the oracle's own account `st` (hmm_oracle_hp.start) of them."""
    cid = start_id(family, n)
    for r in range(st["rounds"]):
        constructed = r == 0 and family in ("ties", "constant", "two_values")
        assert st["ties"][r] == 0 or constructed or float(st["gap"][r]) == 0.0, "%s: round %d has %d exact ties" % (cid, r + 1, st["ties"][r])
        assert float(st["margin"][r]) >= H.MARGIN * float(st["gap"][r]), "%s: round %d decides a window by %.3g of the centre distance" % (
            cid, r + 1, float(st["margin"][r] / st["gap"][r]))
        for shift, thr in st["stop"][r]:
            assert abs(float(shift - thr)) >= STOP_MARGIN * float(thr), "%s: round %d shifts a centre by %.6g of its stop threshold" % (
                cid, r + 1, float(shift / thr))
    if family == "overlap" and n >= SLOW_FROM:
        assert st["rounds"] >= SLOW_ROUNDS, "%s: %d rounds" % (cid, st["rounds"])


def round_conditions(family, n, lls):
    """H.GAP: no round's gain in log-likelihood lies within GAP of the default tol (so that a default fit would stop on the same
    round in every arithmetic)."""
    assert H.gap_from_tol([float(v) for v in lls]) >= H.GAP, "%s: a round's gain is within %g of tol" % (round_id(family, n), H.GAP)


# ---------------------------------------------------------------------------------------------------------------------- the forms
def fit_start(x, native):
    m = H.GaussianHMM2(native=native, n_iter=0).fit(x)
    return m, (m.means_, m.covars_)


def fit_rounds(x, r, native):
    m = H.GaussianHMM2(native=native, n_iter=r, tol=-1e300).fit(x)
    return m, (H.params(m), m.loglik_)


class _NumpyRounds(H.RecordingHMM):
    """The numpy specification, keeping the parameters of every round."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.kept = []

    def _e_step_py(self, x):
        if self.lls:
            self.kept.append((H.params(self), self.lls[-1]))
        return super()._e_step_py(x)


def numpy_rounds(x):
    """{r: (params, loglik)} of the numpy specification for r in ROUNDS, from ONE fit of max(ROUNDS) rounds."""
    m = _NumpyRounds(n_iter=max(ROUNDS), tol=-1e300)
    with np.errstate(divide="ignore"):      # (an outlier's log-space score underflows to log 0 = -inf, which the specification carries)
        m.fit(x)
    m.kept.append((H.params(m), m.lls[-1]))
    return {r: m.kept[r - 1] for r in ROUNDS}
