"""Chosen states for single NMF steps at the shapes where csrc/nmf_kernels.h changes form, and the check of one step's result
against the long-double step of tests/nmf_oracle.py.  Pure numpy, no device: tests/test_nmf_edges_cpu.py qualifies the cases with
two double implementations on the CPU, tests/test_gpu_nmf_edges.py drives the device with them.

Inputs (legacy RandomState streams, elementwise arithmetic and integer sums only, so every machine draws the same bits; a sha256
per case is kept in tests/golden/nmf_edge_cases.json):
  X   multinomial counts of depth 1.2 f per row (48 below f = 40, where sparser rows would miss the few features of a component
      altogether and the shapes are there for their row count) around a mixture sum_t A[s][t] B[t] of d Dirichlet profiles, as proportions:
      non-negative, rows summing to 1, about 30 % exact zeros from f = 40 on.  About a tenth of the columns (at least one where f > 3) are zeroed
      before the rows are normalised, and where n > 3 one row is zero.
  W,H the mixture's own factors, each entry scaled by a uniform factor in [0.8, 1.8) (so that W H matches X in the mean once a quarter is zeroed): positive, near a fixed point of the descent,
      so that a step moves entries both ways; a quarter of the entries of each are then set to exactly 0.
Component states: "none"; "dead0" (H[0,:] = 0 and W[:,0] = 0: dead in both sweeps); "Hlast" (H[d-1,:] = 0, W[:,d-1] alive: the W
sweep meets a zero Hessian and leaves the column, the H sweep revives the row); "Wmid" (W[:,d//2] = 0, H[d//2,:] alive: revived by
the W sweep).

check() is the whole assertion of one step, for whatever produced (W', H', violation):
  * every entry within (1 + 2^-10) x nmf_oracle.step_bound(..., sides=1) of the long-double step (sides = 1: ONE double
    implementation against exact arithmetic; the 2^-10 is the long-double reference's own rounding, as in test_gpu_nmf.py), and the
    violation within its bound;
  * where a bound is 0 (dead components, the frozen H, an all-dead state's violation) the value is exactly the reference's, which
    there is exactly the input;
  * zero pattern: (value == 0) equals (reference == 0) wherever the long-double entry before its max(., 0) is further from 0 than
    the bound.  The entries this leaves out (bound > 0 and |pre| <= bound) are counted outside the all-zero rows (for W) and
    columns (for H) of X and capped at 0.1 % of the entries there; inside them pre is 0 in exact arithmetic for the last live
    component, so nothing is capped there (the value bound holds all the same).
"""
import hashlib
import json
import os
from collections import OrderedDict

import numpy as np

import nmf_oracle as NO

LD = np.longdouble
SLACK = 1 + 2.0 ** -10
LEFT_OUT_CAP = 1e-3
STATES = ("none", "dead0", "Hlast", "Wmid")
HASHES = os.path.join(NO.GOLD, "nmf_edge_cases.json")

# (n, f, d): what the shape reaches.  (8161, 5, 3) is not in the issue's list: it is the smallest n at which XT W inside a step runs
# exactly XTQ_SPLITS = 256 splits (32 rows each, the last of one row); at 8193 the capped split count gives 33 rows and 249 splits.
SHAPES = OrderedDict([
    ((1, 1, 1), "one entry; d = 1 (an all-dead state has violation 0)"),
    ((2, 3, 7), "d above n and f; nmf_sweep<8> below its edge"),
    ((255, 70, 8), "W sweep one row short of a block; nmf_sweep<8> at d = 8"),
    ((256, 64, 9), "W sweep of exactly one block; nmf_sweep<16> at d = 9; f one 64-lane stride"),
    ((257, 65, 16), "W sweep one row into a second block; d at its cap"),
    ((513, 63, 15), "three W blocks, the last of one row; Gram over three strides"),
    ((70, 255, 8), "H sweep one row short of a block"),
    ((64, 256, 9), "H sweep of exactly one block; f = 4 strides"),
    ((65, 257, 4), "H sweep one row into a second block; nmf_sweep<4> at d = 4"),
    ((63, 769, 5), "four H blocks, the last of one row; nmf_sweep<8> at d = 5"),
    ((300, 300, 2), "nmf_sweep<2> at d = 2"),
    ((300, 300, 3), "nmf_sweep<4> at d = 3"),
    ((1025, 40, 6), "five W blocks: the block partials in index order"),
    ((8161, 5, 3), "XT W over exactly 256 row splits, the last of one row; 32 W blocks"),
    ((8193, 6, 2), "XT W at the capped split count (33 rows per split); 33 W blocks"),
    ((1100, 2772, 2), "the CLI's feature count"),
])
# the one shape whose long-double step takes more than a few milliseconds runs one state only
ONE_STATE = {(1100, 2772, 2): [("none", True)]}


def cases(shape):
    return ONE_STATE.get(shape, [(s, u) for s in STATES for u in (True, False)])


def case_id(shape, state, update_H):
    return "n%d_f%d_d%d-%s-%s" % (shape + (state, "WH" if update_H else "W"))


def base(shape):
    """(X, W, H) of a shape before any component state."""
    n, f, d = shape
    rs = np.random.RandomState(7000 + list(SHAPES).index(shape))
    B = np.array([rs.dirichlet(np.full(f, 2.0)) for _ in range(d)])             # d x f profiles
    A = np.array([rs.dirichlet(np.full(d, 0.3)) for _ in range(n)])             # n x d mixing weights, many small
    depth = max(48, int(round(1.2 * f)))
    K = np.zeros((n, f), dtype=np.int64)
    for s in range(n):
        pr = np.zeros(f)
        for t in range(d):
            pr = pr + A[s, t] * B[t]
        K[s] = rs.multinomial(depth, pr)
    if f > 3:
        K[:, rs.choice(f, max(1, int(round(f / 10.0))), replace=False)] = 0
    if n > 3:
        K[rs.randint(n)] = 0
    tot = K.sum(axis=1)
    X = K / np.maximum(tot, 1)[:, None].astype(np.float64)
    W = A * (0.8 + rs.random_sample((n, d)))
    H = B * (0.8 + rs.random_sample((d, f)))
    W[rs.random_sample((n, d)) < 0.25] = 0.0
    H[rs.random_sample((d, f)) < 0.25] = 0.0
    return X, W, H


def with_state(W, H, state):
    W, H = W.copy(), H.copy()
    d = W.shape[1]
    if state == "dead0":
        H[0, :] = 0.0
        W[:, 0] = 0.0
    elif state == "Hlast":
        H[d - 1, :] = 0.0
    elif state == "Wmid":
        W[:, d // 2] = 0.0
    elif state != "none":
        raise ValueError(state)
    return W, H


def digest(X, W, H):
    h = hashlib.sha256()
    for a in (X, W, H):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def recorded_hashes():
    return json.load(open(HASHES))


class Reference:
    """The long-double step from (W, H), its one-sided bounds, and what the zero-pattern rule needs."""

    def __init__(self, X, W, H, update_H):
        self.X, self.W, self.H, self.update_H = X, W, H, update_H
        aux = {}
        self.Wl, self.Hl, self.vl = NO.step(X, W, H, update_H, how="ld", aux=aux)
        bW, bH, bv = NO.step_bound(X, W, H, update_H, sides=1)
        self.bW, self.bH, self.bv = SLACK * bW, SLACK * bH, SLACK * bv
        self.preW, self.gradW = aux["preW"], aux["gradW"]
        self.preH = aux.get("preH", self.Hl)
        self.zero_rows = ~X.any(axis=1)
        self.zero_cols = ~X.any(axis=0)

    def _one(self, got, ref, pre, b, inside):
        """(worst ratio, left out outside, entries outside, left out inside) of one factor."""
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        worst = float(np.max(err[b > 0] / b[b > 0], initial=0.0))
        assert np.all(err <= b), "value outside its bound: worst ratio %.3g, %d entries off where the bound is 0" % (
            worst, int((err[b == 0] > 0).sum()))
        exact = b == 0
        assert np.array_equal(got[exact], ref[exact].astype(np.float64))
        clear = np.abs(pre).astype(np.float64) > b
        assert np.array_equal((got == 0)[clear], (ref == 0)[clear]), "zero pattern differs where |pre| > bound"
        left = ~clear & ~exact
        n_out = int((left & ~inside).sum())
        assert n_out <= LEFT_OUT_CAP * int((~inside).sum()), (n_out, int((~inside).sum()))
        return worst, n_out, int((~inside).sum()), int((left & inside).sum())

    def check(self, W1, H1, v):
        """Assert everything of the module docstring; returns dict(ratio, ratio_v, left_out, outside, left_in)."""
        n, d = self.W.shape
        f = self.H.shape[1]
        assert W1.shape == (n, d) and H1.shape == (d, f) and W1.dtype == np.float64 and H1.dtype == np.float64
        assert np.isfinite(W1).all() and np.isfinite(H1).all() and np.isfinite(v)
        assert W1.min() >= 0 and H1.min() >= 0
        rW = self._one(W1, self.Wl, self.preW, self.bW, np.repeat(self.zero_rows[:, None], d, axis=1))
        rH = self._one(H1, self.Hl, self.preH, self.bH, np.repeat(self.zero_cols[None, :], d, axis=0))
        if not self.update_H:
            assert np.array_equal(H1, self.H) and not self.bH.any()
        ev = abs(float(LD(v) - self.vl))
        assert ev <= self.bv, "violation outside its bound: ratio %.3g" % (ev / self.bv if self.bv else np.inf)
        if self.bv == 0:
            assert v == 0.0
        return {"ratio": max(rW[0], rH[0]), "ratio_v": ev / self.bv if self.bv else 0.0, "left_out": rW[1] + rH[1],
                "outside": rW[2] + rH[2], "left_in": rW[3] + rH[3]}

    def claims(self, state):
        """What the case must really contain (asserted by the CPU qualification)."""
        X, W, H = self.X, self.W, self.H
        n, f = X.shape
        d = W.shape[1]
        assert X.min() >= 0 and X.any() and np.all(np.abs(X.sum(axis=1)[~self.zero_rows] - 1) < 1e-12)
        assert int(self.zero_rows.sum()) == (1 if n > 3 else 0)
        assert int(self.zero_cols.sum()) >= (max(1, int(round(f / 10.0))) if f > 3 else 0)
        if f >= 40:
            assert 0.2 < float((X == 0).mean()) < 0.5
        if state == "none":
            assert n * d < 200 or 0.15 < float((W == 0).mean()) < 0.35
            assert d * f < 200 or 0.15 < float((H == 0).mean()) < 0.35
        assert W.min() >= 0 and H.min() >= 0
        G = (H.astype(LD) @ H.T.astype(LD))
        G2 = (self.Wl.T @ self.Wl)
        if state == "dead0":
            assert G[0, 0] == 0 and not W[:, 0].any() and not self.Wl[:, 0].any() and not self.Hl[0].any() and G2[0, 0] == 0
        elif state == "Hlast":
            assert G[d - 1, d - 1] == 0 and (n <= 3 or W[:, d - 1].any()) and np.array_equal(self.Wl[:, d - 1], W[:, d - 1])
            if self.update_H and n > 3:
                assert G2[d - 1, d - 1] > 0 and self.Hl[d - 1].any()
        elif state == "Wmid":
            assert not W[:, d // 2].any() and (f <= 3 or (H[d // 2].any() and G[d // 2, d // 2] > 0))
            if n > 3:
                assert self.Wl[:, d // 2].any()
        live = np.diag(G).astype(np.float64) != 0
        if n > 3 and live.any():
            # exact zeros of the input on both branches of W[s][t] == 0, in components the sweep does update (g = -X HT <= 0
            # unless a second live component comes with weight: the other branch is claimed where the input has two)
            z = (W == 0) & live[None, :]
            assert (z & (self.gradW < 0)).any() and (z & (self.Wl > 0)).any()
            if int((live & W.any(axis=0)).sum()) > 1:
                assert (z & (self.gradW >= 0) & ~self.zero_rows[:, None]).any() and (z & (self.Wl == 0)).any()
