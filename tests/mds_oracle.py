"""Metric MDS restated in numpy as csrc/mds_kernels.h computes it, with per-entry forward-error bounds.

The GPU computes the dissimilarities D by direct differences, sum_k (x_ik - x_jk)^2 in order, and one SMACOF step as the Guttman
sum over j of ratio_ij (x_i - x_j) / n with direct-difference configuration distances.  sklearn (tools/make_golden_mds.py) computes
D and the configuration distances in the Gram form sqrt(|x_i|^2 - 2 x_i.x_j + |x_j|^2) and the step as (1 / n) B X.  The bounds
below cover both against the exact values:
  D         |D_gpu - D_exact| <= C_D_EXACT F eps D_ij;  |D_gpu - D_sklearn| <= that + min(C_D_GRAM eps s_ij / D_ij, sqrt(C_D_GRAM eps s_ij))
            with s_ij = |x_i|^2 + |x_j|^2 (the Gram form's cancellation);
  one step  |X'_ik - X'_sklearn,ik| <= (C_STEP n eps sum_j |ratio_ij| (|x_i| + |x_j|)      (the cancellation inside B X)
                                       + C_STEP_GRAM eps sum_j D_ij s_ij / dist_ij^2          (sklearn's Gram-form dist_ij)
                                       + sum_j dD_ij) / n                                     (the two D's differ by dD)
            with |x| the row's Euclidean norm;
  stress    from the step bound b_i of each row: sum_ij |e_ij| (b_i + b_j + g_ij) + (b_i + b_j + g_ij)^2, halved, with
            e_ij = dist_ij - D_ij, g_ij = C_D_GRAM eps s_ij / dist_ij + 4 eps dist_ij, plus a relative 1e-13.
The constants are calibrated on the goldens (tests/test_mds_cpu.py reports the worst measured ratio to each bound).

These bounds relate the device to sklearn's Gram form and grow with |x|.  To compare the device with the exact value use
tests/mds_oracle_hp.py (long double, units without a Gram term; tests/test_gpu_mds_edges.py), for which direct_D, step and stress
here serve as the float64 model.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
ZERO_DIST = 1e-5            # sklearn: distances[distances == 0] = 1e-5
C_D_EXACT = 2.0
C_D_GRAM = 16.0
C_STEP = 4.0
C_STEP_GRAM = 16.0


def direct_D(X, rows=None):
    """D[rows] (all rows by default) from direct differences."""
    X = np.asarray(X, dtype=np.float64)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), X.shape[0]))
    for r, i in enumerate(rows):
        out[r] = np.sqrt(((X[i] - X) ** 2).sum(axis=1))
        out[r, i] = 0.0
    return out


def D_bound_exact(D, f):
    return C_D_EXACT * f * EPS * D


def D_bound_gram(X, D, rows=None):
    """The Gram form's extra error on D[rows] (all rows by default)."""
    sq = np.einsum("ij,ij->i", X, X)
    rows = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    s = sq[rows][:, None] + sq[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(D > 0, C_D_GRAM * EPS * s / D, np.inf)
    return np.minimum(rel, np.sqrt(C_D_GRAM * EPS * s))


def distances(Y):
    diff = Y[:, None, :] - Y[None, :, :]
    return np.sqrt((diff * diff).sum(-1))


def stress(Y, D):
    """sklearn's raw stress: sum over all i, j of (dist_ij - D_ij)^2 / 2, and the sum of dist_ij^2 / 2 of its stop rule."""
    dist = distances(Y)
    return float(((dist - D) ** 2).sum() / 2), float((dist ** 2).sum() / 2)


def step(Y, D):
    """X_{t+1} from X_t = Y as the GPU computes it: (1 / n) sum_j ratio_ij (y_i - y_j), ratio_ij = D_ij / dist_ij (1e-5 for an
    exact 0)."""
    n = Y.shape[0]
    diff = Y[:, None, :] - Y[None, :, :]
    dist = np.sqrt((diff * diff).sum(-1))
    ratio = D / np.where(dist == 0.0, ZERO_DIST, dist)
    np.fill_diagonal(ratio, 0.0)
    return np.einsum("ij,ijk->ik", ratio, diff) * (1.0 / n)


def step_bound(Y, D, dD=0.0):
    """Per-row bound (n x 1, the same for every column) of one step from Y against sklearn's step on a D that differs by dD."""
    n = Y.shape[0]
    dist = distances(Y)
    safe = np.where(dist == 0.0, ZERO_DIST, dist)
    ratio = D / safe
    np.fill_diagonal(ratio, 0.0)
    norm = np.sqrt((Y * Y).sum(axis=1))
    sq = norm * norm
    s = sq[:, None] + sq[None, :]
    cancel = C_STEP * n * EPS * (ratio * (norm[:, None] + norm[None, :])).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        gram = np.where(dist > 0, C_STEP_GRAM * EPS * D * s / (dist * dist), 0.0).sum(axis=1)
    dD = np.broadcast_to(np.asarray(dD, dtype=np.float64), D.shape)
    return ((cancel + gram + dD.sum(axis=1)) / n)[:, None]


def stress_bound(Y, D, b):
    """Bound on the stress of Y when every entry of row i is within b_i (n x 1) of Y, the distances computed either way."""
    dist = distances(Y)
    sq = (Y * Y).sum(axis=1)
    s = sq[:, None] + sq[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(dist > 0, C_D_GRAM * EPS * s / dist, np.sqrt(C_D_GRAM * EPS * s)) + 4 * EPS * dist
    bb = np.sqrt(Y.shape[1]) * (b[:, 0][:, None] + b[:, 0][None, :]) + g
    np.fill_diagonal(bb, 0.0)
    e = np.abs(dist - D)
    st = ((dist - D) ** 2).sum() / 2
    return float((e * bb + bb * bb).sum() / 2 + 1e-13 * st)
