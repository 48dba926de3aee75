"""numpy restatement of the route frisk_amd.projection.IncrementalPCA takes (sklearn's IncrementalPCA.partial_fit with the SVD of
the stacked matrix A replaced by the eigendecomposition of G = AT A), and the helpers the IncrementalPCA tests share: the regenerated
inputs, the sign alignment and the tolerance ratios.  Test infrastructure: it imports neither sklearn nor the package under test."""
import hashlib
import json
import os

import numpy as np

from golden_util import GOLD

TOL = 1e-9                  # Y, components: of max|golden|; scalars: relative; noise_variance_: of explained_variance_[0]
SIGN_MARGIN = 1e-6          # below it the sign of a component is rounding's choice: compared up to sign

G = json.load(open(os.path.join(GOLD, "ipca.json"))) if os.path.exists(os.path.join(GOLD, "ipca.json")) else None


def arrays(case):
    return np.load(os.path.join(GOLD, "ipca", G["cases"][case]["file"]))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def make_X(spec):
    """The case's input, regenerated as tools/make_golden_mds.py make_X draws it (legacy RandomState streams are frozen)."""
    rs = np.random.RandomState(spec["seed"])
    n = spec["n"]
    sizes = [n // 3 + (1 if b < n % 3 else 0) for b in range(3)]
    rows = []
    for m in sizes:
        centre = [rs.dirichlet(np.full(w, 2.0)) for w in spec["orders"]]
        for _ in range(m):
            rows.append(np.concatenate([rs.dirichlet(c * spec["spread"] + 1e-3) for c in centre]))
    return np.array(rows)[rs.permutation(n)]


def X_of(case):
    X = make_X(G["cases"][case]["X"])
    assert sha(X) == G["cases"][case]["X"]["sha256"]
    return X


def gen_batches(n, batch_size, min_batch_size):
    out, start = [], 0
    for _ in range(int(n // batch_size)):
        end = start + batch_size
        if end + min_batch_size > n:
            continue
        out.append((start, end))
        start = end
    if start < n:
        out.append((start, n))
    return out


def mean_var_update(Xb, seen, mean, var):
    """sklearn's _incremental_mean_and_var (no NaN, no weights)."""
    b = Xb.shape[0]
    new_sum = Xb.sum(axis=0)
    total = seen + b
    T = new_sum / b
    temp = Xb - T
    correction = temp.sum(axis=0)
    new_unnorm = (temp ** 2).sum(axis=0) - correction ** 2 / b
    if seen == 0:
        return new_sum / total, new_unnorm / total, T
    last_sum = mean * seen
    ratio = seen / b
    upd = var * seen + new_unnorm + ratio / total * (last_sum / ratio - new_sum) ** 2
    return (last_sum + new_sum) / total, upd / total, T


def stacked(Xb, st, mean_new, T):
    if st is None:
        return Xb - mean_new
    b, seen = Xb.shape[0], st["n"]
    corr = np.sqrt((seen / (seen + b)) * b) * (st["mean"] - T)
    return np.vstack((st["S"].reshape(-1, 1) * st["Vt"], Xb - T, corr))


def sign_rule(comps):
    big = np.argmax(np.abs(comps), axis=1)
    return comps * np.sign(comps[np.arange(comps.shape[0]), big])[:, None]


def partial_fit(st, Xb, d):
    """One batch from the state st (None: unfitted): the new state {n, mean, var, S, Vt, ev, evr, noise}."""
    b, f = Xb.shape
    seen = 0 if st is None else st["n"]
    mean, var, T = mean_var_update(Xb, seen, None if st is None else st["mean"], None if st is None else st["var"])
    A = stacked(Xb, st, mean, T)
    Gm = A.T @ A
    Gm = np.triu(Gm) + np.triu(Gm, 1).T
    w, v = np.linalg.eigh(Gm)
    order = np.argsort(w, kind="stable")[::-1][:d]
    lam = np.maximum(w[order], 0.0)
    S = np.sqrt(lam)
    total = seen + b
    m = min(A.shape[0], f)
    nxt = np.sort(w)[::-1][:d + 1]
    gap = float(np.min(nxt[:-1] - nxt[1:]) / nxt[0]) if len(nxt) > 1 else np.inf
    noise = 0.0 if d in (b, f) else max(float(np.trace(Gm)) - float(lam.sum()), 0.0) / (total - 1) / (m - d)
    return {"n": total, "mean": mean, "var": var, "S": S, "Vt": sign_rule(v[:, order].T.copy()), "ev": S ** 2 / (total - 1),
            "evr": S ** 2 / np.sum(var * total), "noise": noise, "gap": gap}


def state_of(a, k, n_seen):
    """sklearn's recorded state after batch k of a case's arrays."""
    return {"n": n_seen, "mean": a["mean_%d" % k], "var": a["var_%d" % k], "S": a["S_%d" % k], "Vt": a["comps_%d" % k],
            "ev": a["ev_%d" % k], "evr": a["evr_%d" % k], "noise": float(a["noise"][k])}


def transform(X, st):
    return (X - st["mean"]) @ st["Vt"].T


def signs_for(got_Vt, want_Vt, margins):
    """+1 for every component whose recorded sign margin pins the sign; else the sign that aligns got with want."""
    s = np.ones(len(want_Vt))
    for i, m in enumerate(margins):
        if m < SIGN_MARGIN and float(got_Vt[i] @ want_Vt[i]) < 0.0:
            s[i] = -1.0
    return s


def ratios(got, want, margins):
    """Worst |got - want| over its tolerance, per quantity, of two states (dicts as partial_fit returns)."""
    s = signs_for(got["Vt"], want["Vt"], margins)
    out = {"comps": float(np.max(np.abs(got["Vt"] * s[:, None] - want["Vt"])) / (TOL * np.max(np.abs(want["Vt"]))))}
    for key in ("mean", "var", "S", "ev", "evr"):
        g, w = np.asarray(got[key], dtype=np.float64), np.asarray(want[key], dtype=np.float64)
        den = np.where(w == 0.0, 1.0, np.abs(w))
        out[key] = float(np.max(np.abs(g - w) / (TOL * den)))
    out["noise"] = abs(got["noise"] - want["noise"]) / (TOL * want["ev"][0])
    return out, s


def y_ratio(Y, want, s=None):
    if s is not None:
        Y = Y * s[None, :]
    return float(np.max(np.abs(Y - want)) / (TOL * np.max(np.abs(want))))


def pca_Y(X, d):
    """The PCA of X (what an alias of pca() would return): for the distance of a multi-batch fit from it."""
    Xc = X - X.mean(axis=0)
    Gm = Xc.T @ Xc
    w, v = np.linalg.eigh(np.triu(Gm) + np.triu(Gm, 1).T)
    order = np.argsort(w, kind="stable")[::-1][:d]
    return Xc @ sign_rule(v[:, order].T.copy()).T


def distance_up_to_sign(Y, Z):
    """max over columns of min(|y - z|, |y + z|), over max|Z|."""
    return max(min(np.max(np.abs(Y[:, q] - Z[:, q])), np.max(np.abs(Y[:, q] + Z[:, q]))) for q in range(Y.shape[1])) / np.max(np.abs(Z))
