"""Shapes, inputs and the comparison of the per-entry IncrementalPCA tests (tests/test_ipca_hp_cpu.py, tests/test_gpu_ipca_edges.py,
tools/make_golden_ipca_hp.py)  --  TEST INFRASTRUCTURE.  Seeded; depends on numpy only.

A case is one batch: (group, b, f, d, seen, family).  seen = 0 is a first batch; a later batch starts from a state (mean, var, S,
Vt) that the tests install with set_state.  The shapes are the smallest at which each piece of ipca_kernels.h can go wrong:

  first_b      b around rows_per / nsplit (64 row ranges) and rows_pad (multiples of 16), and 4033 = 64 * 63 + 1
  first_f      f around the 256-column blocks of the one-thread-per-column kernels and the 64-column Gram tiles
  first_f2772  990 tiles, rows_pad 48 / 64 / 80: G on 48 sampled columns
  first_cap    f = 8: rows_pad / 16 below, at and above the 2048-block cap of the K split
  first_dff    d = f
  later_rows   d + b + 1 on and just past a multiple of 16
  later_b1     a batch shorter than d
  later_d      d head rows, 1 .. 64, at f = 70
  later_f257, later_f2772

Families of inputs:
  kmer       Dirichlet blobs around three centres, the distribution of ipca_oracle.make_X (blocks of k-mer proportions of orders
             1..6, each summing to 1), rows of the three blobs mixed
  offset     1 + 1e-6 * normal: column offset 1, spread 1e-6
  zeroconst  kmer with column 0 all zero and the last column constant 0.25.  A power of two on purpose: its sums are exact in any
             order, so the column must come out as exactly zero in A.  A constant such as 0.3 drifts systematically in a serial
             float64 sum (343 eps at 4033 rows in numpy's), which is second order in G (b dT^2) yet 26 000 units of that entry:
             it would set the one tolerance that every other entry of every case is held to
  sspan      kmer, the state's (and the committed) singular values spanning 1e3 .. 1e-3
  unperm     later batches only: the state from one blob, the batch from another, so |mean_old - T| is comparable to the column
             spread and the correction row and the variance's cross term carry an O(1) share (assert_shares)
The state of a later batch is that of d + 8 earlier rows of the same family (their mean, variance and SVD), whatever `seen` says.

compare() is the one comparison every test uses: worst |got - oracle| / unit per quantity (units: tests/ipca_oracle_hp.py);
check() asserts it against the tolerance of tests/golden/ipca_hp.json.  restate() is the float64 restatement of
tests/ipca_oracle.py, clean or with one of seven planted defects.
"""
import collections
import functools
import json
import os
import zlib

import numpy as np

import ipca_oracle as IO
import ipca_oracle_hp as HP
from golden_util import GOLD

JSON = os.path.join(GOLD, "ipca_hp.json")
FACTOR = 8                      # tolerance = FACTOR * worst ratio of the float64 restatement (as the KLD and HMM pins)
DEFECT_MARGIN = 10              # every planted defect exceeds a tolerance by this factor on some case
QUANTITIES = ("G", "mean", "var", "Y")
SEEN = (1, 7, 100000)
ORDERS = (2, 10, 32, 136, 512, 2080)
FOREIGN = 5                     # rows outside the batch that the transform of a case also takes
MEAN_SPLITS = 64                # row ranges of the column sums (proj_kernels.h), for defect g
DEFECTS = ("a_no_correction_row", "b_mean_new_for_T", "c_head_without_S", "d_coef_b_over_total", "e_last_row_lost",
           "f_var_over_new_count", "g_colsum_skips_last_split")

Case = collections.namedtuple("Case", "id group b f d seen family")


def golden():
    with open(JSON) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------------------------ the list
def _cases():
    first = [("first_b", b, 9, 1 if b == 1 else 2) for b in (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4033)]
    first += [("first_f", 40, f, min(f, 2)) for f in (1, 2, 63, 64, 65, 255, 256, 257)]
    first += [("first_f2772", b, 2772, 2) for b in (48, 49, 64, 65)]
    first += [("first_cap", b, 8, 2) for b in (32752, 32768, 32769)]
    first += [("first_dff", 12, 5, 5)]
    later = [("later_rows", rows - 3, 9, 2) for rows in (16, 17, 32, 33)]
    later += [("later_b1", 1, 9, 3)]
    later += [("later_d", 20, 70, d) for d in (1, 2, 3, 64)]
    later += [("later_f257", 40, 257, 2)]
    out = []
    for group, b, f, d in first:
        for fam in ("kmer", "offset", "zeroconst", "sspan"):
            out.append(Case("%s/b%d_f%d_d%d/%s" % (group, b, f, d, fam), group, b, f, d, 0, fam))
    for group, b, f, d in later:
        for seen in SEEN:
            for fam in ("kmer", "offset", "zeroconst", "sspan", "unperm"):
                out.append(Case("%s/b%d_f%d_d%d_seen%d/%s" % (group, b, f, d, seen, fam), group, b, f, d, seen, fam))
    for k, fam in enumerate(("kmer", "offset", "zeroconst", "sspan", "unperm", "unperm")):
        seen = SEEN[k % 3]
        out.append(Case("later_f2772/b61_f2772_d2_seen%d/%s" % (seen, fam), "later_f2772", 61, 2772, 2, seen, fam))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
MP_CASES = ("first_b/b15_f9_d2/kmer", "first_dff/b12_f5_d5/offset", "later_rows/b13_f9_d2_seen7/unperm")


def sample_cols(f):
    """All columns up to f = 257; at f = 2772, 48: the first, the last, both sides of multiples of 64 and of the 256-column
    blocks, and seeded others."""
    if f <= 257:
        return None
    fixed = [0, f - 1, 63, 64, 127, 128, 255, 256, 257, 2047, 2048, 2687, 2688, 2751, 2752, f - 2]
    rs = np.random.RandomState(f)
    rest = [c for c in rs.permutation(f).tolist() if c not in fixed][:48 - len(fixed)]
    return np.array(sorted(fixed + rest), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------ inputs
def orders_of(f):
    out, left = [], f
    for w in ORDERS:
        if left < w:
            break
        out.append(w)
        left -= w
    return out + ([left] if left else [])


def _blobs(rs, f):
    return [np.concatenate([rs.dirichlet(np.full(w, 2.0)) if w > 1 else np.ones(1) for w in orders_of(f)]) for _ in range(3)]


def _draw(rs, centres, which, f, spread=60.0):
    """Rows around centres[which[r]]: per block a Dirichlet(centre * spread + 1e-3) draw (a normalised gamma vector)."""
    g = rs.standard_gamma(np.array(centres)[which] * spread + 1e-3)
    lo = 0
    for w in orders_of(f):
        g[:, lo:lo + w] /= g[:, lo:lo + w].sum(axis=1, keepdims=True)
        lo += w
    return g


def _orthonormal(rs, d, f):
    q, _ = np.linalg.qr(rs.standard_normal((f, d)))
    return np.ascontiguousarray(q.T)


Inputs = collections.namedtuple("Inputs", "Xb state foreign S_new Vt_new")


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(Xb, state or None, foreign rows, S_new, Vt_new): the batch, the state before it ({n, mean, var, S, Vt}), FOREIGN rows for
    the transform, and the decomposition the tests commit (a fixed orthonormal Vt_new)."""
    c = BY_ID[case_id]
    rs = np.random.RandomState(zlib.crc32(case_id.encode()))
    n_prev = c.d + 8
    n = n_prev + c.b + FOREIGN
    if c.family == "offset":
        rows = 1.0 + 1e-6 * rs.standard_normal((n, c.f))
    else:
        centres = _blobs(rs, c.f)
        if c.family == "unperm":
            which = np.concatenate((np.zeros(n_prev, int), np.full(c.b, 2), np.ones(FOREIGN, int)))
        else:
            which = rs.randint(0, 3, n)
        rows = _draw(rs, centres, which, c.f)
        if c.family == "zeroconst":
            rows[:, -1] = 0.25
            rows[:, 0] = 0.0
    prev, Xb, foreign = rows[:n_prev], np.ascontiguousarray(rows[n_prev:n_prev + c.b]), np.ascontiguousarray(rows[n_prev + c.b:])
    span = np.geomspace(1e3, 1e-3, c.d) if c.d > 1 else np.array([1e3])
    state = None
    if c.seen:
        mean = prev.mean(axis=0)
        _u, s, vt = np.linalg.svd(prev - mean, full_matrices=False)
        state = {"n": c.seen, "mean": mean, "var": prev.var(axis=0), "S": span if c.family == "sspan" else s[:c.d].copy(),
                 "Vt": np.ascontiguousarray(vt[:c.d])}
    S_new = span if c.family == "sspan" else np.linspace(2.0, 1.0, c.d)
    return Inputs(Xb, state, foreign, S_new, _orthonormal(rs, c.d, c.f))


def transform_rows(case_id):
    i = inputs(case_id)
    return np.vstack((i.Xb, i.foreign))


@functools.lru_cache(maxsize=None)
def oracle(case_id):
    """The long-double results of a case and their units: batch() of tests/ipca_oracle_hp.py (G on sample_cols) plus Y, u_Y of the
    batch and the foreign rows under (the oracle's new mean, Vt_new)."""
    c, i = BY_ID[case_id], inputs(case_id)
    st = i.state or {"n": 0, "mean": None, "var": None, "S": None, "Vt": None}
    o = HP.batch(i.Xb, st["n"], st["mean"], st["var"], st["S"], st["Vt"], cols=sample_cols(c.f))
    o["Y"], o["u_Y"] = HP.transform(transform_rows(case_id), o["mean"], i.Vt_new)
    del o["A"]
    return o


# ------------------------------------------------------------------------------------------------------------------ comparison
def compare(case_id, got):
    """{quantity: worst |got - oracle| / unit} for the quantities present in got (G: the full f x f matrix; mean, var; Y of
    transform_rows)."""
    o = oracle(case_id)
    out = {}
    for q in QUANTITIES:
        if q in got:
            g = np.asarray(got[q], dtype=np.float64)
            if q == "G" and sample_cols(BY_ID[case_id].f) is not None:
                g = g[sample_cols(BY_ID[case_id].f), :]
            assert g.shape == o[q].shape, (case_id, q, g.shape, o[q].shape)
            out[q] = HP.ratio(g, o[q], o["u_" + q])
    return out


def check(case_id, got, tolerance, what=""):
    r = compare(case_id, got)
    bad = {q: "%.3g > %.3g" % (v, tolerance[q]) for q, v in r.items() if not v <= tolerance[q]}
    assert not bad, "%s %s: |got - oracle| / unit over the tolerance: %s" % (case_id, what, bad)
    return r


def assert_shares(minimum=0.10):
    """The unpermuted later batches put at least `minimum` of trace G into the correction row and of the summed variance into the
    merge's cross term, in at least one case each; returns the two best (share, case)."""
    corr = max((oracle(c.id)["corr_share"], c.id) for c in CASES if c.family == "unperm")
    cross = max((oracle(c.id)["cross_share"], c.id) for c in CASES if c.family == "unperm")
    assert corr[0] >= minimum and cross[0] >= minimum, (corr, cross)
    return corr, cross


# ------------------------------------------------------------------------------------------------------------------ restatement
def _planted(Xb, st, defect):
    """mean_var_update + stacked of tests/ipca_oracle.py, operation for operation, with one defect planted (None: none - asserted
    bit-identical to tests/ipca_oracle.py by tests/test_ipca_hp_cpu.py)."""
    b = Xb.shape[0]
    seen = 0 if st is None else st["n"]
    if defect == "g_colsum_skips_last_split":
        rows_per = (b + MEAN_SPLITS - 1) // MEAN_SPLITS
        nsplit = (b + rows_per - 1) // rows_per
        new_sum = Xb[:(nsplit - 1) * rows_per].sum(axis=0)
    else:
        new_sum = Xb.sum(axis=0)
    total = seen + b
    T = new_sum / b
    temp = Xb - T
    correction = temp.sum(axis=0)
    new_unnorm = (temp ** 2).sum(axis=0) - correction ** 2 / b
    if seen == 0:
        mean, var = new_sum / total, new_unnorm / total
        A = Xb - mean
    else:
        last_sum = st["mean"] * seen
        ratio = seen / b
        upd = st["var"] * seen + new_unnorm + ratio / total * (last_sum / ratio - new_sum) ** 2
        mean, var = (last_sum + new_sum) / total, upd / (b if defect == "f_var_over_new_count" else total)
        coef = np.sqrt(((b if defect == "d_coef_b_over_total" else seen) / (seen + b)) * b)
        head = st["Vt"].copy() if defect == "c_head_without_S" else st["S"].reshape(-1, 1) * st["Vt"]
        mid = Xb - (mean if defect == "b_mean_new_for_T" else T)
        A = np.vstack((head, mid, coef * (st["mean"] - T)))
        if defect == "a_no_correction_row":
            A = A[:-1]
    if defect == "e_last_row_lost":
        A = A.copy()
        A[(0 if seen == 0 else len(st["S"])) + b - 1] = 0.0
    return mean, var, T, A


def restate(case_id, defect=None):
    """{G, mean, var, Y} of the float64 restatement (tests/ipca_oracle.py: mean_var_update, stacked, A.T @ A, transform)."""
    i = inputs(case_id)
    if defect is None:
        seen = 0 if i.state is None else i.state["n"]
        mean, var, T = IO.mean_var_update(i.Xb, seen, None if i.state is None else i.state["mean"],
                                          None if i.state is None else i.state["var"])
        A = IO.stacked(i.Xb, i.state, mean, T)
    else:
        mean, var, T, A = _planted(i.Xb, i.state, defect)
    return {"G": A.T @ A, "mean": mean, "var": var, "Y": IO.transform(transform_rows(case_id), {"mean": mean, "Vt": i.Vt_new})}
